"""STOI micro-benchmark (run on the GPU box): metrics.stoi_batch on 256 clean/processed clip pairs of 1-10 s at 16 kHz
(the whole batch: upload, resample to 10 kHz, silent-frame removal, band envelopes, correlations, one synchronisation),
timed with HIP events, next to the float64 CPU oracle's time per clip (tests/stoi_reference.py) and the largest score
difference between the two."""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sos_amd  # noqa: E402,F401
from sos_amd import metrics  # noqa: E402
import stoi_reference as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--oracle-clips", type=int, default=8, help="clips the CPU oracle scores (time per clip, parity)")
    args = ap.parse_args()
    fs = 16000
    rng = np.random.default_rng(7)
    lens = rng.integers(1 * fs, 10 * fs + 1, size=args.clips)
    noise = rng.uniform(0.002, 0.5, size=args.clips)
    pairs = [R.closed_form_pair(1000 + 2 * i, int(n), fs, float(s)) for i, (n, s) in enumerate(zip(lens, noise))]
    xs = [torch.from_numpy(p[0]).cuda() for p in pairs]
    ys = [torch.from_numpy(p[1]).cuda() for p in pairs]
    audio_s = float(lens.sum()) / fs
    for extended in (False, True):
        scores = metrics.stoi_batch(xs, ys, fs, extended)        # warm-up: code objects, filter taps
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            metrics.stoi_batch(xs, ys, fs, extended)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / args.iters
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ref = [R.stoi(pairs[i][0], pairs[i][1], fs, extended) for i in range(args.oracle_clips)]
        cpu_s = (time.perf_counter() - t0) / args.oracle_clips
        err = max(abs(scores[i] - ref[i]) for i in range(args.oracle_clips))
        name = "ESTOI" if extended else "STOI "
        print(f"{name} {args.clips} clips ({audio_s:.0f} s of audio at 16 kHz): GPU batch {ms:8.3f} ms "
              f"({audio_s / (ms / 1e3):9.0f} x real time); CPU f64 oracle {cpu_s * 1e3:8.1f} ms per clip "
              f"(x {args.clips} = {cpu_s * args.clips:6.1f} s); max |GPU - oracle| over {args.oracle_clips} clips {err:.1e}")


if __name__ == "__main__":
    main()
