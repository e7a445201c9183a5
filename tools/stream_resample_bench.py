"""Streaming-resampler benchmark (run on the GPU box): audio_io.StreamResampler at 48 kHz -> 14 kHz in chunks of 100 ms, for 1,
16 and 64 slots in lock step, all streams in their steady state.  Per slot count, --runs times alternating between
  * the launch pair of one push (sos_stream_push_f32 + sos_stream_resample_f32, resident tables) between HIP events, and the
    second launch alone at each tile shape of --tiles (SOS_STREAM_RESAMPLE_TILE: outputs per workgroup step),
  * the same audio as one clip per slot through audio_io.resample_batch_device in one call,
  * a float4 copy (torch's copy kernel) of the bytes the stream kernel moves (the ring samples it reads, the outputs it writes),
  * the host's wall time of a whole StreamResampler.push of those chunks;
then a pipeline.StreamDenoiser step with and without in_sr=48000, out_sr=48000 at tools/stream_bench.py's geometry (fp16, cores
of 2 s + 0.5 s context, chunks of 100 ms), alternating.  One line per figure.
--high-band measures the band merge of live audio instead: the sos_stream_band_merge_f32 launch ('keep', 'follow') against the
output resampler's sos_stream_resample_f32 launch on a step's outputs, the ring state per slot, and a StreamDenoiser step at
48 kHz under high_band = 'drop' (twice), 'keep' and 'follow', alternating."""
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


def band_kernels(args):
    """--high-band: the merge launch of one step's output (audio_io.StreamBandMerger, 'keep' and 'follow') against the
    sos_stream_resample_f32 launch of the output resampler on the same outputs, and the ring state per slot."""
    from sos_amd import tools
    hop, lib = 158, L.lib()
    chunk14 = int(round(args.chunk * SR))
    for slots in args.slots:
        lag = 4 * chunk14
        x = torch.randn((slots, 14 * chunk14 * IN_SR // SR + 64), device="cuda")
        a = torch.stack([audio_io.resample_device(x[s], IN_SR, SR) for s in range(slots)])
        b = 0.5 * a
        rs = audio_io.StreamResampler(slots, SR, IN_SR, max_chunk=chunk14)
        mergers = {"keep": audio_io.StreamBandMerger(slots, SR, IN_SR, lag, gains=None, hop=hop, max_chunk=4 * chunk14),
                   "follow": audio_io.StreamBandMerger(slots, SR, IN_SR, lag, gains=2, hop=hop, max_chunk=4 * chunk14)}
        n_x = lambda m: min(int(m * IN_SR / SR), x.shape[1])      # noqa: E731
        for k in range(10):                                     # ten pushes in: every stream is in its steady state
            lo, hi = k * chunk14, (k + 1) * chunk14
            rs.push({s: b[s, lo:hi] for s in range(slots)})
            for mg in mergers.values():
                mg.push({s: (x[s, n_x(lo):n_x(hi)], a[s, lo:hi], b[s, lo:hi]) for s in range(slots)})
        # the rows of the next push, resident: running them again and again rewrites the same outputs
        m0, m1 = 10 * chunk14, 11 * chunk14
        t0, t1 = rs.t_done[0], rs._ready(m1)[0]
        fill = [(s, s * chunk14, chunk14, m0) for s in range(slots)]
        tools.stream_push(b[:, m0:m1].contiguous().reshape(-1), fill, rs.ring)
        rows = np.ascontiguousarray(np.asarray([(s, t0, t1, m1, t1, s * (t1 - t0)) for s in range(slots)], dtype=np.int64))
        d_rows = torch.from_numpy(rows).cuda()
        out = torch.empty(slots * (t1 - t0), device="cuda")

        def resample():
            L.check(lib.sos_stream_resample_f32(L.ptr(rs.ring), slots, rs.capacity, L.ptr(d_rows), rows.ctypes.data, slots, rs.ratio,
                                                L.ptr(rs.win), rs.win.numel(), rs.num_table, L.ptr(out), out.numel(), L.stream_ptr()))

        calls, told = {}, {}
        for name, mg in mergers.items():
            K = mg.smooth
            ring3 = mg.ring.view(3, slots, mg.capacity)
            for plane, src, lo, hi in ((0, x, n_x(m0), n_x(m1)), (1, a, m0, m1), (2, b, m0, m1)):      # the next chunk into the rings
                tools.stream_push(src[:, lo:hi].contiguous().reshape(-1), [(s, s * (hi - lo), hi - lo, lo) for s in range(slots)],
                                  ring3[plane])
            u0, (u1, _, _) = mg.t_done[0], mg._ready(m1, n_x(m1))
            r_hi = m1 // hop
            if K is not None:
                tools.stream_band_ratio(mg.ring, mg.rring, [(s, mg.r_hi[s], r_hi, m1, m1) for s in range(slots)], hop)
            mrows = np.ascontiguousarray(np.asarray([(s, u0, u1, n_x(m1), m1, m1, u1, -1, r_hi, s * (u1 - u0)) for s in range(slots)],
                                                    dtype=np.int64))
            d_mrows = torch.from_numpy(mrows).cuda()
            rrows = np.ascontiguousarray(np.asarray([(s, m0 // hop, r_hi, m1, m1) for s in range(slots)], dtype=np.int64))
            d_rrows = torch.from_numpy(rrows).cuda()
            mout = torch.empty(slots * (u1 - u0), device="cuda")

            def merge(mg=mg, K=K, mrows=mrows, d_mrows=d_mrows, mout=mout):
                L.check(lib.sos_stream_band_merge_f32(L.ptr(mg.ring), slots, mg.capacity, L.ptr(mg.rring), mg.frames, L.ptr(d_mrows),
                                                      mrows.ctypes.data, slots, mg.ratio, L.ptr(mg.win), mg.win.numel(), mg.num_table,
                                                      hop, -1 if K is None else K, L.ptr(mout), mout.numel(), L.stream_ptr()))

            def ratio(mg=mg, rrows=rrows, d_rrows=d_rrows):
                L.check(lib.sos_stream_band_ratio_f64(L.ptr(mg.ring), slots, mg.capacity, L.ptr(d_rrows), rrows.ctypes.data, slots, hop,
                                                      L.ptr(mg.rring), mg.frames, L.stream_ptr()))

            calls[name] = (merge, ratio if K is not None else None)
            told[name] = (u1 - u0, 12 * mg.capacity + 8 * mg.frames)
        # the bytes a merge launch moves per slot: 2 R + the chunk of a and of b, the outputs' x, the outputs
        floats = slots * (2 * (chunk14 + 2 * rs.R) + 2 * (t1 - t0))
        src, dst = torch.empty(floats // 2, device="cuda"), torch.empty(floats // 2, device="cuda")
        for run in range(args.runs):
            ms_rs = _timed(resample, args.iters)
            ms = {name: (_timed(m, args.iters), _timed(r, args.iters) if r else None) for name, (m, r) in calls.items()}
            ms_copy = _timed(lambda: dst.copy_(src), args.iters)
            print(f"{slots:3d} slots x {args.chunk * 1e3:g} ms at {SR} -> {IN_SR} Hz, run {run}: sos_stream_resample_f32 of {t1 - t0} outputs "
                  f"per slot {ms_rs * 1e3:8.1f} us; sos_stream_band_merge_f32 'keep' of {told['keep'][0]} {ms['keep'][0] * 1e3:8.1f} us, "
                  f"'follow' of {told['follow'][0]} {ms['follow'][0] * 1e3:8.1f} us; sos_stream_band_ratio_f64 of {chunk14 // hop} frames "
                  f"{ms['follow'][1] * 1e3:8.1f} us; float4 copy of the {4 * floats / 1e6:.3f} MB a merge launch moves "
                  f"{ms_copy * 1e3:6.1f} us; ring state per slot at max_lag {lag}: keep {told['keep'][1]} bytes, follow "
                  f"{told['follow'][1]} bytes")


def band_denoiser(args):
    """--high-band: a StreamDenoiser step at in_sr = out_sr = 48 kHz under 'drop' (twice: its own run-to-run spread), 'keep' and
    'follow', alternating."""
    det, jm = _nets()
    kw = dict(window_seconds=2.0, context_seconds=0.5, in_sr=IN_SR, out_sr=IN_SR)
    n, chunk = int(args.seconds * SR), int(round(args.chunk * IN_SR))
    for slots in args.slots:
        base = [_wave(900 + i, n * IN_SR // SR) for i in range(4)]
        audio48 = torch.stack([torch.roll(base[s % 4], 1009 * (s // 4)) for s in range(slots)])
        made = {name: pipeline.StreamDenoiser(det, jm, slots, high_band=mode, **kw)
                for name, mode in (("drop", "drop"), ("drop again", "drop"), ("keep", "keep"), ("follow", "follow"))}
        for sd in made.values():
            _session(sd, audio48, chunk)                        # warm-up
        for name in ("keep", "follow"):
            mg = made[name].merger
            print(f"{slots:3d} slots, high_band='{name}': merger rings of {mg.capacity} samples, {12 * mg.capacity + 8 * mg.frames} bytes "
                  f"per slot (max_lag {mg.max_lag})")
        for run in range(args.runs):
            for name, sd in made.items():                       # the four alternate
                wall, steps, idle, got = _session(sd, audio48, chunk)
                print(f"{slots:3d} slots x {args.seconds:g} s, fp16, 2 s cores + 0.5 s context, {args.chunk * 1e3:g} ms chunks at 48 kHz, run "
                      f"{run}, StreamDenoiser high_band {name}: {len(steps)} steps, median {np.median(steps):8.2f} ms per step (min "
                      f"{min(steps):.2f}, max {max(steps):.2f}); {len(idle)} other pushes, median {np.median(idle):.3f} ms of host time; "
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
    ap.add_argument("--high-band", action="store_true",
                    help="measure the band merge of live audio (StreamBandMerger, StreamDenoiser(high_band=)) instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_resample_bench needs an MI355X: nothing is measured without one")
    with torch.no_grad():
        (band_kernels if args.high_band else kernels)(args)
        if not args.no_denoiser:
            sos_amd.set_precision("fp16")
            try:
                (band_denoiser if args.high_band else denoiser)(args)
            finally:
                sos_amd.set_precision("bf16")


if __name__ == "__main__":
    main()
