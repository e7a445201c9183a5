"""Streaming-resampler benchmark (run on the GPU box): audio_io.StreamResampler at 48 kHz -> 14 kHz in chunks of 100 ms, for 1,
16 and 64 slots in lock step, all streams in their steady state.  Per slot count, --runs times alternating between
  * the launch pair of one push (sos_stream_push_f32 + sos_stream_resample_f32, resident tables) between HIP events, and the
    second launch alone at each tile shape of --tiles (SOS_STREAM_RESAMPLE_TILE: outputs per workgroup step),
  * the same audio as one clip per slot through audio_io.resample_batch_device in one call,
  * a float4 copy (torch's copy kernel) of the bytes the stream kernel moves (the ring samples it reads, the outputs it writes),
  * the host's wall time of a whole StreamResampler.push of those chunks;
then a pipeline.StreamDenoiser step with and without in_sr=48000, out_sr=48000 at tools/stream_bench.py's geometry (fp16, cores
of 2 s + 0.5 s context, chunks of 100 ms), alternating.  One line per figure."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sos_amd  # noqa: E402
from sos_amd import _lib as L  # noqa: E402
from sos_amd import audio_io, pipeline  # noqa: E402
from stream_bench import _nets, _session, _timed, _wave  # noqa: E402

IN_SR, SR = 48000, 14000


def kernels(args):
    chunk = int(round(args.chunk * IN_SR))
    lib = L.lib()
    for slots in args.slots:
        rs = audio_io.StreamResampler(slots, IN_SR, SR, max_chunk=chunk)
        x = torch.randn((slots, 12 * chunk), device="cuda")
        for k in range(10):                                     # ten pushes in: every stream is in its steady state
            rs.push({s: x[s, k * chunk:(k + 1) * chunk] for s in range(slots)})
        # the tables of the next push, resident; running them again and again rewrites the same ring samples and outputs
        n0, t0, flat = rs.n_recv[0], rs.t_done[0], x[:, 10 * chunk:11 * chunk].contiguous().reshape(-1)
        t1 = rs._ready(n0 + chunk)[0]
        fill = np.ascontiguousarray(np.asarray([(s, s * chunk, chunk, n0) for s in range(slots)], dtype=np.int64))
        rows = np.ascontiguousarray(np.asarray([(s, t0, t1, n0 + chunk, t1, s * (t1 - t0)) for s in range(slots)], dtype=np.int64))
        d_fill, d_rows = torch.from_numpy(fill).cuda(), torch.from_numpy(rows).cuda()
        out = torch.empty(slots * (t1 - t0), device="cuda")

        def push():
            L.check(lib.sos_stream_push_f32(L.ptr(flat), flat.numel(), L.ptr(d_fill), fill.ctypes.data, slots, L.ptr(rs.ring), slots,
                                            rs.capacity, L.stream_ptr()))

        def resample():
            L.check(lib.sos_stream_resample_f32(L.ptr(rs.ring), slots, rs.capacity, L.ptr(d_rows), rows.ctypes.data, slots, rs.ratio,
                                                L.ptr(rs.win), rs.win.numel(), rs.num_table, L.ptr(out), out.numel(), L.stream_ptr()))

        def pair():
            push()
            resample()

        clips = [x[s, :11 * chunk][-(chunk + 2 * rs.R):].contiguous() for s in range(slots)]   # the samples the stream kernel reads
        whole = [x[s, 10 * chunk:11 * chunk].contiguous() for s in range(slots)]
        floats = slots * (chunk + 2 * rs.R + (t1 - t0))
        src, dst = torch.empty(floats // 2, device="cuda"), torch.empty(floats // 2, device="cuda")
        sessions = [audio_io.StreamResampler(slots, IN_SR, SR, max_chunk=chunk) for _ in range(args.runs)]
        for run in range(args.runs):
            ms_pair = _timed(pair, args.iters)
            ms_tile = {}
            for tile in args.tiles:
                os.environ["SOS_STREAM_RESAMPLE_TILE"] = str(tile)
                ms_tile[tile] = _timed(resample, args.iters)
            os.environ.pop("SOS_STREAM_RESAMPLE_TILE", None)
            ms_batch = _timed(lambda: audio_io.resample_batch_device(whole, IN_SR, SR), max(args.iters // 10, 3))
            ms_wings = _timed(lambda: audio_io.resample_batch_device(clips, IN_SR, SR), max(args.iters // 10, 3))
            ms_copy = _timed(lambda: dst.copy_(src), args.iters)
            sr_run = sessions[run]
            sr_run.push({s: x[s, :chunk] for s in range(slots)})
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            for k in range(1, 11):
                sr_run.push({s: x[s, k * chunk:(k + 1) * chunk] for s in range(slots)})
            host = (time.perf_counter() - w0) / 10 * 1e3
            torch.cuda.synchronize()
            print(f"{slots:3d} slots x {args.chunk * 1e3:g} ms at {IN_SR} -> {SR} Hz ({chunk} samples in, {t1 - t0} out per slot), run {run}: "
                  f"push + resample launches {ms_pair * 1e3:8.1f} us; resample alone at tile "
                  + ", ".join(f"{t}: {ms_tile[t] * 1e3:.1f} us" for t in args.tiles)
                  + f"; resample_batch_device of the chunks as clips {ms_batch * 1e3:8.1f} us (with their wings {ms_wings * 1e3:.1f} us); "
                  f"float4 copy of the {4 * floats / 1e6:.3f} MB the stream kernel moves {ms_copy * 1e3:6.1f} us; "
                  f"StreamResampler.push host time {host * 1e3:8.1f} us")


def denoiser(args):
    det, jm = _nets()
    kw = dict(window_seconds=2.0, context_seconds=0.5)
    n = int(args.seconds * SR)
    for slots in args.slots:
        base = [_wave(900 + i, n * IN_SR // SR) for i in range(4)]
        audio48 = torch.stack([torch.roll(base[s % 4], 1009 * (s // 4)) for s in range(slots)])
        audio14 = torch.stack([audio_io.resample_device(a, IN_SR, SR)[:n] for a in audio48])
        made = {"at 14 kHz": (pipeline.StreamDenoiser(det, jm, slots, **kw), audio14, int(round(args.chunk * SR))),
                "in_sr = out_sr = 48 kHz": (pipeline.StreamDenoiser(det, jm, slots, in_sr=IN_SR, out_sr=IN_SR, **kw), audio48,
                                            int(round(args.chunk * IN_SR)))}
        for sd, audio, chunk in made.values():
            _session(sd, audio, chunk)                          # warm-up
        for run in range(args.runs):
            for name, (sd, audio, chunk) in made.items():       # the two alternate
                wall, steps, idle, got = _session(sd, audio, chunk)
                print(f"{slots:3d} slots x {args.seconds:g} s, fp16, 2 s cores + 0.5 s context, {args.chunk * 1e3:g} ms chunks, run {run}, "
                      f"StreamDenoiser {name}: {len(steps)} steps, median {np.median(steps):8.2f} ms per step (min {min(steps):.2f}, max "
                      f"{max(steps):.2f}); {len(idle)} other pushes, median {np.median(idle):.3f} ms of host time; "
                      f"{slots * args.seconds / wall:8.1f} s of audio per second ({got} samples out)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--chunk", type=float, default=0.1, help="seconds of audio per slot and push")
    ap.add_argument("--seconds", type=float, default=20.0, help="audio per slot of the StreamDenoiser sessions")
    ap.add_argument("--tiles", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--runs", type=int, default=3, help="alternating runs of the variants")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-denoiser", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_resample_bench needs an MI355X: nothing is measured without one")
    with torch.no_grad():
        kernels(args)
        if not args.no_denoiser:
            sos_amd.set_precision("fp16")
            try:
                denoiser(args)
            finally:
                sos_amd.set_precision("bf16")


if __name__ == "__main__":
    main()
