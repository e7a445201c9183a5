"""Silent-interval labeller micro-benchmark (run on the GPU box): labels.silence_bits_batch on 256 clips of 1-10 s already on
the device (the whole call: concatenation, table upload, launch sequence, one download, host split) against the loop of
one-clip calls, at 14 kHz and at 44.1 kHz, timed with HIP events; and the launch sequence alone on resident buffers, whose
time bounds the energy kernel's from above: the bytes that kernel must read (4 per sample) and write (8 per frame) over that
time, next to the HBM peak.  The kernels' own times come from a kernel trace of this program in a run of its own."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sos_amd  # noqa: E402,F401
from sos_amd import labels  # noqa: E402
import silence_reference as R  # noqa: E402

HBM_PEAK = 8.0e12               # bytes/s, MI355X specification; a float4 copy reaches about 6.3e12


def _timed(fn, iters):
    fn()                                                        # warm-up: code objects, the allocator's blocks
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--loop-iters", type=int, default=2)
    ap.add_argument("--fps", type=float, default=30.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_bench needs an MI355X: nothing is measured without one")
    for sr in (14000, 44100):
        rng = np.random.default_rng(7)
        lens = rng.integers(1 * sr, 10 * sr + 1, size=args.clips)
        host = [R.speechlike(3000 + i, n / sr, sr) for i, n in enumerate(lens)]
        xs = [torch.from_numpy(x).cuda() for x in host]
        samples = float(sum(len(x) for x in host))
        want = labels.silence_bits_batch(xs, sr, args.fps)
        frames = float(sum(len(b) for b in want))
        loop = [labels.silence_bits(x, sr, args.fps) for x in xs]
        assert all(np.array_equal(a, b) for a, b in zip(want, loop))
        ref = [R.label_seconds(host[i], sr, args.fps) for i in range(4)]
        assert all(r["undecided"] > 0 or np.array_equal(r["bits"], want[i]) for i, r in enumerate(ref))
        ms_batch = _timed(lambda: labels.silence_bits_batch(xs, sr, args.fps), args.iters)
        ms_loop = _timed(lambda: [labels.silence_bits(x, sr, args.fps) for x in xs], args.loop_iters)
        st = labels._stage(xs, [sr] * len(xs), [args.fps] * len(xs), 40.0, 0.1, 0.0, 0.0)
        ms_seq = _timed(lambda: labels._launch(st), 10 * args.iters)
        nbytes = 4.0 * samples + 8.0 * frames
        print(f"{sr} Hz: {args.clips} clips, {samples / sr:.0f} s of audio, {frames:.0f} frames at {args.fps:g} fps")
        print(f"  silence_bits_batch {ms_batch:8.3f} ms per call ({args.clips / (ms_batch / 1e3):9.0f} clips/s); loop of one-clip "
              f"calls {ms_loop:8.3f} ms ({args.clips / (ms_loop / 1e3):9.0f} clips/s): {ms_loop / ms_batch:.1f} x")
        print(f"  launch sequence on resident clips (energy + label kernels) {ms_seq * 1e3:8.1f} us: the energy kernel's "
              f"{nbytes / 1e6:.1f} MB in at least {nbytes / (ms_seq / 1e3) / 1e12:.2f} TB/s (HBM peak {HBM_PEAK / 1e12:.1f} TB/s: "
              f"{100 * nbytes / (ms_seq / 1e3) / HBM_PEAK:.0f} %)")


if __name__ == "__main__":
    main()
