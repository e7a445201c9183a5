"""Noisy-speech synthesis micro-benchmark (run on the GPU box): tools.add_signals_ragged on 256 clips of 1-10 s at 14 kHz
already on the device (the whole call: concatenation, table uploads, launch sequence, the wait for the status rows) against the
loop of 256 one-clip tools.add_signals_batch calls (sos_add_signals_f32, one workgroup per clip: the baseline), timed with HIP
events; and the launch sequence alone on resident buffers, as a rate over the bytes the algorithm needs (two f32 reads and three
f32 writes per sample, plus the frame decisions) next to the streaming rate of a float4 copy.  The kernels' own times come
from a kernel trace of this program in a run of its own."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sos_amd  # noqa: E402,F401
from sos_amd import ragged, tools  # noqa: E402
import mix_reference as R  # noqa: E402
import silence_reference as S  # noqa: E402

STREAM = 6.3e12                 # bytes/s a float4 copy reaches on an MI355X (HBM specification: 8.0e12)


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
    ap.add_argument("--snr", type=float, default=3.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench needs an MI355X: nothing is measured without one")
    sr = 14000
    rng = np.random.default_rng(7)
    lens = rng.integers(1 * sr, 10 * sr + 1, size=args.clips)
    host = [S.speechlike(3000 + i, n / sr, sr) for i, n in enumerate(lens)]
    recording = (0.1 * rng.standard_normal(12 * sr)).astype(np.float32)          # one noise recording, a crop per clip
    starts = [int(rng.integers(0, len(recording) - n + 1)) for n in lens]
    xs = [torch.from_numpy(x).cuda() for x in host]
    d_rec = torch.from_numpy(recording).cuda()
    samples = float(sum(len(x) for x in host))
    index = [0] * args.clips
    for with_bits in (False, True):
        bits = ratios = None
        frames = 0.0
        if with_bits:
            bits = [torch.from_numpy(rng.integers(0, 2, int(round(n / sr * args.fps))).astype(np.uint8)).cuda() for n in lens]
            ratios = sr / args.fps
            frames = float(sum(b.numel() for b in bits))
        kw = dict(noise_index=index, starts=starts, bits=bits, ratios=ratios)
        mixed, clean, noise, detail = tools.add_signals_ragged(xs, [d_rec], args.snr, return_detail=True, **kw)
        for i in range(3):                                       # the results are the restatement's before anything is timed
            ref = R.mix(host[i], recording, args.snr, start=starts[i], bits=None if bits is None else bits[i].cpu().numpy(),
                        ratio=ratios)
            err = float(np.max(np.abs(mixed[i].cpu().numpy() - ref["mixed"])))
            assert err <= R.OUT_TOL * np.max(np.abs(ref["mixed"])), (i, err)
        ms_call = _timed(lambda: tools.add_signals_ragged(xs, [d_rec], args.snr, **kw), args.iters)
        lens_l, nlens, crop, par, nb = tools._mix_plan(xs, [d_rec], args.snr, index, starts, None, bits, ratios, 0.5)
        ntab = np.ascontiguousarray(np.stack([crop[:, 1], crop[:, 2]], axis=1))
        st = tools._mix_stage(xs, ragged.concat([d_rec])[0], len(recording), ntab, par, bits, nb, 0.5)
        ms_seq = _timed(lambda: tools._mix_launch(st), 10 * args.iters)
        nbytes = 20.0 * samples + frames
        print(f"{args.clips} clips, {samples / sr:.0f} s of audio at {sr} Hz, " +
              (f"{frames:.0f} frame decisions at {args.fps:g} fps" if with_bits else "no frame decisions"))
        print(f"  add_signals_ragged {ms_call:8.3f} ms per call ({args.clips / (ms_call / 1e3):9.0f} clips/s)")
        print(f"  launch sequence on resident clips (plan, energies, peaks, outputs) {ms_seq * 1e3:8.1f} us: "
              f"{nbytes / 1e6:.1f} MB the algorithm needs at {nbytes / (ms_seq / 1e3) / 1e12:.2f} TB/s (a float4 copy streams "
              f"{STREAM / 1e12:.1f} TB/s: {100 * nbytes / (ms_seq / 1e3) / STREAM:.0f} %)")
        if not with_bits:
            # the baseline: one clip per sos_add_signals_f32 call, the crop taken on the device
            def loop():
                for x, s0 in zip(xs, starts):
                    tools.add_signals_batch(x[None], d_rec[s0:s0 + x.numel()][None], args.snr)
            one = tools.add_signals_batch(xs[0][None], d_rec[starts[0]:starts[0] + xs[0].numel()][None], args.snr)[0][0]
            dev = float((one - mixed[0]).abs().max())
            assert dev <= 2 * R.OUT_TOL * 0.5, dev                # both within OUT_TOL of the restatement at peak 0.5
            ms_loop = _timed(loop, args.loop_iters)
            print(f"  loop of one-clip add_signals_batch calls {ms_loop:8.3f} ms ({args.clips / (ms_loop / 1e3):9.0f} clips/s): "
                  f"{ms_loop / ms_call:.2f} x the ragged call's time")


if __name__ == "__main__":
    main()
