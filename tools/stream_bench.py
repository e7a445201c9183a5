"""Streaming benchmark (run on the GPU box): pipeline.StreamDenoiser with 1, 16 and 64 slots in lock step, cores of 2 s with
0.5 s of context, fp16, fed in chunks of 100 ms of synthetic noisy speech (dataset.synth_batch; four distinct recordings,
rotated for the further slots) for 60 s per slot.  Per slot count, --runs times alternating between the eager session and
graph=True (after one warm-up session each, which also captures the graphs):
  * the time of a step -- a push() that runs one window per slot -- between HIP events around that call, median over the run,
  * the host's wall time of the other push() calls (chunks that complete no window),
  * seconds of audio denoised per second of wall time over the whole session (the last synchronisation included),
and once the same audio through pipeline.denoise_long with the same windows (the offline reference, HIP events around whole
calls).  Then the stage and stitch kernels alone on the 64 slots' inner windows, resident buffers, as a rate over the bytes they
move next to a float4 copy (torch's copy kernel) of the same number of bytes.  One line per configuration."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sos_amd  # noqa: E402
from oracle import nets as onet  # noqa: E402
from sos_amd import _lib as L  # noqa: E402
from sos_amd import pipeline, tools, windows  # noqa: E402

SR = 14000


def _wave(seed, n):
    from sos_amd.dataset import synth_batch
    parts = synth_batch(seed, (n + 27999) // 28000)["mixed"]
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(list(parts))[:n])).cuda()


def _nets():
    from sos_amd.common import MyConfig
    from sos_amd.denoiser import networks as jnet
    from sos_amd.detector import networks as dnet
    det = dnet.get_network()
    det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    return det.cuda().eval(), jm.cuda().eval()


def _timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _session(sd, audio, chunk):
    """One whole session: every slot gets its next `chunk` samples per call, then all are closed.
    -> (wall seconds, [ms of each step between HIP events], [host ms of each other push], output samples)."""
    slots, n = audio.shape
    steps, idle, events, got = [], [], [], 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for at in range(0, n, chunk):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t1 = time.perf_counter()
        a.record()
        out = sd.push({s: audio[s, at:at + chunk] for s in range(slots)})
        b.record()
        t2 = time.perf_counter()
        if out[0].numel():
            events.append((a, b))
        else:
            idle.append((t2 - t1) * 1e3)
        got += sum(int(o.numel()) for o in out.values())
    got += sum(int(o.numel()) for o in sd.close(list(range(slots))).values())
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    steps = [a.elapsed_time(b) for a, b in events]
    return wall, steps, idle, got


def sessions(args, det, jm):
    n, chunk = int(args.seconds * SR), int(round(args.chunk * SR))
    base = [_wave(900 + i, n) for i in range(4)]
    kw = dict(window_seconds=args.window, context_seconds=args.context)
    for slots in args.slots:
        audio = torch.stack([torch.roll(base[s % 4], 1009 * (s // 4)) for s in range(slots)])
        made = {graph: pipeline.StreamDenoiser(det, jm, slots, graph=graph, **kw) for graph in (False, True)}
        for sd in made.values():
            _session(sd, audio, chunk)                          # warm-up: plans, tables, workspaces, graph captures
        for run in range(args.runs):
            for graph, sd in made.items():                      # the two alternate
                wall, steps, idle, got = _session(sd, audio, chunk)
                print(f"{slots:3d} slots x {args.seconds:g} s, {args.precision}, {args.window:g} s cores + {args.context:g} s context, "
                      f"{args.chunk * 1e3:g} ms chunks, run {run}, {'graph=True' if graph else 'eager     '}: {len(steps)} steps, median "
                      f"{np.median(steps):8.2f} ms per step (min {min(steps):.2f}, max {max(steps):.2f}); {len(idle)} other pushes, median "
                      f"{np.median(idle):.3f} ms of host time; {slots * args.seconds / wall:8.1f} s of audio per second ({wall:.3f} s "
                      f"wall, {got} samples out, {made[True].captures} graphs)")
        clips = list(audio)
        ms = _timed(lambda: pipeline.denoise_long(det, jm, clips, **kw), args.iters)
        print(f"{slots:3d} slots x {args.seconds:g} s, {args.precision}: the same audio through denoise_long, the same windows {ms:9.1f} ms per call "
              f"({slots * args.seconds / (ms / 1e3):8.1f} s of audio per second)")


def kernels(args):
    slots = max(args.slots)
    core, context = windows._hops(round(args.window * SR)), windows._hops(round(args.context * SR))
    cap, m = 2 * core + context, core + 2 * context
    ring, tail = torch.randn((slots, cap), device="cuda"), torch.randn((slots, 2, 2 * context), device="cuda")
    stage = np.ascontiguousarray(np.asarray([(s, 5 * core - context, m) for s in range(slots)], dtype=np.int64))
    stitch = np.ascontiguousarray(np.asarray([(s, s, 5 * core - context, m, 5 * core, 6 * core, 3, 0) for s in range(slots)], dtype=np.int64))
    rows = tools.stream_stage(ring, stage, m)
    out, _ = tools.stream_stitch(rows, stitch, context, tail)
    d_stage, d_stitch = torch.from_numpy(stage).cuda(), torch.from_numpy(stitch).cuda()
    lib = L.lib()
    ms_stage = _timed(lambda: L.check(lib.sos_stream_stage_f32(L.ptr(ring), slots, cap, L.ptr(d_stage), stage.ctypes.data, slots, m,
                                                               L.ptr(rows), L.stream_ptr())), 200)
    ms_stitch = _timed(lambda: L.check(lib.sos_stream_stitch_f32(L.ptr(rows), slots, m, L.ptr(d_stitch), stitch.ctypes.data, slots, slots,
                                                                 context, L.ptr(tail), L.ptr(out), core, L.stream_ptr())), 200)
    for name, ms, floats in (("sos_stream_stage_f32", ms_stage, 2 * slots * m), ("sos_stream_stitch_f32", ms_stitch, slots * (2 * core + 6 * context))):
        src, dst = torch.empty(floats // 2, device="cuda"), torch.empty(floats // 2, device="cuda")
        ms_copy = _timed(lambda: dst.copy_(src), 200)
        nbytes = 4.0 * floats
        print(f"{name} ({slots} inner windows of {args.window:g} s + 2 x {args.context:g} s, resident buffers): {ms * 1e3:8.1f} us, "
              f"{nbytes / 1e6:.2f} MB at {nbytes / (ms / 1e3) / 1e12:.3f} TB/s; a float4 copy of the same bytes {ms_copy * 1e3:8.1f} us "
              f"({nbytes / (ms_copy / 1e3) / 1e12:.3f} TB/s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--seconds", type=float, default=60.0, help="audio per slot")
    ap.add_argument("--chunk", type=float, default=0.1, help="seconds of audio per slot and push")
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--context", type=float, default=0.5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--runs", type=int, default=3, help="alternating runs of the eager and the graphed session")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-sessions", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs an MI355X: nothing is measured without one")
    det, jm = _nets()
    sos_amd.set_precision(args.precision)
    try:
        with torch.no_grad():
            if not args.no_sessions:
                sessions(args, det, jm)
            kernels(args)
    finally:
        sos_amd.set_precision("bf16")


if __name__ == "__main__":
    main()
