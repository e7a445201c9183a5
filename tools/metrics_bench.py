"""Evaluation micro-benchmark (run on the GPU box): metrics.evaluate_metrics_batch on 256 (noisy, clean) pairs of 1-10 s at
16 kHz (the generator of tests/test_metrics.py) against the loop of metrics.evaluate_metrics over the same clips, once with
numpy inputs (upload included) and once with GPU tensors.  The two are alternated in one process after a warm-up of both;
each timing is a host clock around a call that ends with the device drained.  Prints ms per batch, multiples of real time,
the ratio loop / batch with its spread over the repetitions, and the largest relative difference between the two on each key.
--batch-only runs the batch alone (for `rocprofv3 --kernel-trace --stats -- python tools/metrics_bench.py --batch-only`)."""
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
from test_metrics import signals  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-only", action="store_true")
    args = ap.parse_args()
    if args.reps < 3 and not args.batch_only:
        ap.error("--reps: at least three repetitions (the spread is part of the result)")
    sr = 16000
    lens = np.random.default_rng(7).integers(1 * sr, 10 * sr + 1, size=args.clips)
    pairs = [signals(1000 + 2 * i, int(n), sr) for i, n in enumerate(lens)]
    audio_s = float(lens.sum()) / sr
    inputs = {"numpy": ([p[1] for p in pairs], [p[0] for p in pairs])}
    inputs["gpu tensors"] = ([torch.from_numpy(n).cuda() for n in inputs["numpy"][0]],
                             [torch.from_numpy(c).cuda() for c in inputs["numpy"][1]])

    def batch(noisy, clean):
        return metrics.evaluate_metrics_batch(noisy, clean, sr=sr)

    def loop(noisy, clean):
        return [metrics.evaluate_metrics(n, c, sr=sr) for n, c in zip(noisy, clean)]

    warnings.simplefilter("ignore", RuntimeWarning)
    print(f"{args.clips} clips, {audio_s:.0f} s of audio at {sr} Hz")
    if args.batch_only:
        for kind, (noisy, clean) in inputs.items():
            batch(noisy, clean)
            ms = [timed(lambda: batch(noisy, clean))[0] for _ in range(args.reps)]
            print(f"{kind:12s} batch {min(ms):9.2f} ms (best of {args.reps})")
        return
    for kind, (noisy, clean) in inputs.items():
        batch(noisy[:4], clean[:4])                     # warm-up: code objects, window and filter tables
        loop(noisy[:4], clean[:4])
        tb, tl = [], []
        for _ in range(args.reps):
            ms, rb = timed(lambda: batch(noisy, clean))
            tb.append(ms)
            ms, rl = timed(lambda: loop(noisy, clean))
            tl.append(ms)
        ratios = [a / b for a, b in zip(tl, tb)]
        print(f"{kind:12s} batch {np.median(tb):9.2f} ms [{min(tb):.2f} .. {max(tb):.2f}] ({audio_s / (np.median(tb) / 1e3):8.0f} x real time)"
              f"   loop {np.median(tl):9.2f} ms [{min(tl):.2f} .. {max(tl):.2f}] ({audio_s / (np.median(tl) / 1e3):8.0f} x real time)"
              f"   loop / batch {np.median(ratios):6.2f} [{min(ratios):.2f} .. {max(ratios):.2f}] over {args.reps} repetitions")
        diffs = []
        for k in rb[0]:
            vals = [(b[k], l[k]) for b, l in zip(rb, rl)]
            if all(b is None and l is None for b, l in vals):
                diffs.append(f"{k} None")
            else:
                diffs.append(f"{k} {max(abs(b - l) / (abs(l) + 1e-12) for b, l in vals):.1e}")
        print(f"{'':12s} largest relative difference batch vs loop: " + ", ".join(diffs))


if __name__ == "__main__":
    main()
