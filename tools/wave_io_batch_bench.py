"""Batched wave front door benchmark (run on the GPU box): 256 clips of 1 .. 10 s with seeded lengths, resampled
14 -> 16 kHz (the evaluation's resample in handoff.denoise_files) and 44.1 -> 14 kHz (loading), once by the loop of
audio_io.resample_device over the clips and once by one audio_io.resample_batch_device call.  Loop and batch alternate,
three repeats each (more with --repeats); the medians, the spread of the repeats and the ratio are printed.
--threads 256,512,1024 also times the batch kernel at those workgroup sizes (SOS_RESAMPLE_BATCH_THREADS; the results do not
depend on it)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sos_amd  # noqa: E402,F401
from sos_amd import audio_io  # noqa: E402


def once(fn):
    """Wall time of one call, in ms, from an idle device to an idle device (launch overhead of the loop included)."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", default="", help="comma-separated workgroup sizes of the batch kernel to time as well")
    args = ap.parse_args()
    sizes = [int(t) for t in args.threads.split(",") if t]
    print(torch.cuda.get_device_name(0))
    for orig, target in ((14000, 16000), (44100, 14000)):
        rng = np.random.default_rng(orig)
        lens = rng.integers(orig, 10 * orig + 1, size=args.clips)
        clips = [torch.randn(int(n), device="cuda") for n in lens]
        loop = lambda: [audio_io.resample_device(c, orig, target) for c in clips]          # noqa: E731
        batch = lambda: audio_io.resample_batch_device(clips, orig, target)                  # noqa: E731
        ref, got = loop(), batch()                                                           # warm-up, and the same bits
        assert all(torch.equal(r, g) for r, g in zip(ref, got))
        del ref, got
        t_loop, t_batch, t_size = [], [], {t: [] for t in sizes}
        for _ in range(args.repeats):
            t_loop.append(once(loop))
            t_batch.append(once(batch))
            for t in sizes:
                os.environ["SOS_RESAMPLE_BATCH_THREADS"] = str(t)
                try:
                    t_size[t].append(once(batch))
                finally:
                    del os.environ["SOS_RESAMPLE_BATCH_THREADS"]
        ml, mb = float(np.median(t_loop)), float(np.median(t_batch))
        secs = float(lens.sum()) / orig
        print(f"{orig} -> {target} Hz, {args.clips} clips, {secs:.0f} s of audio: loop {ml:8.2f} ms (min {min(t_loop):.2f}, max "
              f"{max(t_loop):.2f})   batch {mb:8.2f} ms (min {min(t_batch):.2f}, max {max(t_batch):.2f})   loop / batch = {ml / mb:.2f}")
        for t in sizes:
            print(f"    batch kernel with {t:4d} threads per workgroup: {float(np.median(t_size[t])):8.2f} ms "
                  f"(min {min(t_size[t]):.2f}, max {max(t_size[t]):.2f})")


if __name__ == "__main__":
    main()
