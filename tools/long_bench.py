"""Long-recording benchmark (run on the GPU box): one synthetic recording (default 10 minutes at 14 kHz, dataset.synth_batch
pieces back to back) denoised whole by pipeline.denoise_ragged([clip]) and in overlapping windows by pipeline.denoise_long at
several window lengths, in fp16, timed with HIP events around whole calls, peak memory from the allocator; the two window
kernels alone (sos_window_stage_f32, sos_window_stitch_f32) on the recording's 30 s plan, as a rate over the bytes they move,
next to a float4 copy (torch's copy kernel) of the same number of bytes.  --distance: how far the windowed result is from the
whole-file result on a 60 s recording with the closed-form test networks in bf16x3 -- a characterisation of random-weight
networks, nothing is asserted on it.  One line per configuration.
--decisions: denoise_long(stitch_bits=True) -- one detector pass over all windows, one decision stream per recording, then the
`bits=` path -- next to the default on the same recording; the `bits=` path on a mixed batch (the recording plus 63 recordings
of 2 s) with time and peak memory; and the two kernels of that path alone (sos_window_stage_masked_f32,
sos_window_frames_stitch_f32) as a rate next to a float4 copy of the same bytes.  --root CHECKOUT runs this script's lines on
another checkout of the repository (its package and its built libraries), e.g. the parent commit for the `bits=` line:
    python tools/long_bench.py --no-speed --decisions --root ../parent
--signals: the four signals of the hand-off on the same mixed batch: sos_window_stitch_planes_f32 (4 planes, file-major, one
launch) against the sequence it replaces -- four sos_window_stitch_f32 launches and one sos_ragged_unpack_f32 launch over every
output sample -- alternating, --signal-runs times each, next to a float4 copy of the one launch's bytes; the file-major launch
with pitches that leave segments off 16-byte boundaries; and denoise_long(bits=, signals=True) next to the plain `bits=` call."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv[1:-1]:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import sos_amd  # noqa: E402
from oracle import nets as onet  # noqa: E402
from sos_amd import _lib as L  # noqa: E402
from sos_amd import pipeline, tools, transform  # noqa: E402
try:
    from sos_amd import windows  # noqa: E402
except ImportError:                 # --root: a checkout from before the windowed layer had a module of its own
    windows = pipeline

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
    """(ms per call, peak bytes allocated during the timed calls) after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, torch.cuda.max_memory_allocated()


def speed(args, det, jm):
    n = int(args.seconds * SR)
    clip = _wave(800, n)
    sos_amd.set_precision(args.precision)
    try:
        if not args.skip_whole:
            ms, peak = _timed(lambda: pipeline.denoise_ragged(det, jm, [clip]), args.iters)
            print(f"{args.seconds:g} s at {SR} Hz, {args.precision}: whole file, denoise_ragged([clip])      {ms:9.1f} ms per call "
                  f"({args.seconds / (ms / 1e3):7.1f} x real time), peak {peak / 2**30:6.2f} GiB")
        for win, cols in [(w, 65536) for w in args.windows] + [(30.0, c) for c in args.max_columns]:
            plan = pipeline.window_plan([n], round(win * SR), round(args.context * SR))
            groups = len(pipeline._length_groups(plan[:, 2].tolist(), 256, cols))
            ms, peak = _timed(lambda: pipeline.denoise_long(det, jm, [clip], window_seconds=win, context_seconds=args.context,
                                                            max_columns=cols), args.iters)
            print(f"{args.seconds:g} s at {SR} Hz, {args.precision}: denoise_long, {win:g} s windows + {args.context:g} s context "
                  f"({len(plan):3d} windows, max_columns {cols}: {groups} groups) {ms:9.1f} ms per call "
                  f"({args.seconds / (ms / 1e3):7.1f} x real time), peak {peak / 2**30:6.2f} GiB")
    finally:
        sos_amd.set_precision("bf16")
    # the two kernels alone, on resident buffers
    hop = transform.HOP_LENGTH
    context = windows._hops(round(args.context * SR))
    plan = np.ascontiguousarray(pipeline.window_plan([n], round(30.0 * SR), context))
    stride = int(plan[:, 2].max())
    rows = tools.window_stage(clip, plan, stride)
    held = plan.copy()
    held[:, 2] = hop * (plan[:, 2] // hop)                      # what a window's row holds
    out = tools.window_stitch(rows, held, context)
    d_plan, d_held = torch.from_numpy(plan).cuda(), torch.from_numpy(held).cuda()
    lib = L.lib()
    ms_stage, _ = _timed(lambda: L.check(lib.sos_window_stage_f32(L.ptr(clip), clip.numel(), L.ptr(d_plan), plan.ctypes.data, len(plan),
                                                                  stride, L.ptr(rows), L.stream_ptr())), 200)
    ms_stitch, _ = _timed(lambda: L.check(lib.sos_window_stitch_f32(L.ptr(rows), len(plan), stride, L.ptr(d_held), held.ctypes.data,
                                                                    len(plan), context, L.ptr(out), L.stream_ptr())), 200)
    n_out = int((plan[:, 5] - plan[:, 4]).sum())
    for name, ms, floats_in, floats_out in (("sos_window_stage_f32", ms_stage, int(plan[:, 2].sum()), rows.numel()),
                                            ("sos_window_stitch_f32", ms_stitch, n_out + 2 * context * (len(plan) - 1), n_out)):
        src, dst = torch.empty((floats_in + floats_out) // 2, device="cuda"), torch.empty((floats_in + floats_out) // 2, device="cuda")
        ms_copy, _ = _timed(lambda: dst.copy_(src), 200)
        nbytes = 4.0 * (floats_in + floats_out)
        print(f"{name} ({len(plan)} windows of 30 s + {args.context:g} s, resident buffers): {ms * 1e3:8.1f} us, "
              f"{nbytes / 1e6:.1f} MB at {nbytes / (ms / 1e3) / 1e12:.3f} TB/s; a float4 copy of the same bytes {ms_copy * 1e3:8.1f} us "
              f"({nbytes / (ms_copy / 1e3) / 1e12:.3f} TB/s)")


def decisions(args, det, jm):
    n = int(args.seconds * SR)
    clip = _wave(800, n)
    shorts = [_wave(801 + i, 2 * SR) for i in range(63)]
    rng = np.random.default_rng(14)
    mixed = [clip] + shorts
    bits = [torch.from_numpy(rng.integers(0, 2, pipeline.n_video_frames(c.numel())).astype(np.uint8)).cuda() for c in mixed]
    new = hasattr(pipeline, "detect_long")
    kw = dict(window_seconds=30.0, context_seconds=args.context)
    sos_amd.set_precision(args.precision)
    try:
        if new and not args.kernels_only:
            for name, fn in (("default (each window silenced by its own detector pass)", lambda: pipeline.denoise_long(det, jm, [clip], **kw)),
                             ("stitch_bits=True (one decision stream per recording)", lambda: pipeline.denoise_long(det, jm, [clip], stitch_bits=True, **kw)),
                             ("detect_long alone", lambda: pipeline.detect_long(det, [clip], **kw))):
                ms, peak = _timed(fn, args.iters)
                print(f"{args.seconds:g} s at {SR} Hz, {args.precision}, 30 s windows: {name} {ms:9.1f} ms per call, peak {peak / 2**30:6.2f} GiB")
        if not args.kernels_only:
            for name, cl, bt in (("the recording alone", [clip], bits[:1]), ("the recording + 63 recordings of 2 s", mixed, bits)):
                ms, peak = _timed(lambda: pipeline.denoise_long(None, jm, cl, bits=bt, fps=30.0, **kw), args.iters)
                print(f"{args.seconds:g} s at {SR} Hz, {args.precision}, 30 s windows: bits= path, {name} {ms:9.1f} ms per call, "
                      f"peak {peak / 2**30:6.2f} GiB (inputs resident: {sum(c.numel() for c in cl) * 4 / 2**30:.3f} GiB)")
    finally:
        sos_amd.set_precision("bf16")
    if not new:
        return
    # the two kernels alone, on resident buffers: the mixed batch's plan
    from sos_amd import ragged
    ns = [int(c.numel()) for c in mixed]
    core, context = windows._hops(round(30.0 * SR)), windows._hops(round(args.context * SR))
    plan = np.ascontiguousarray(pipeline.window_plan(ns, core, context))
    stride, W = int(plan[:, 2].max()), len(plan)
    flat, d_bits = torch.cat(mixed), torch.cat(bits)
    clips = ragged.clip_table(ns, [len(b) for b in bits])
    rat = np.full(len(ns), SR / 30.0)
    wave, masked = tools.window_stage_masked(flat, d_bits, clips, rat, plan, stride)
    d_plan, d_clips, d_rat = torch.from_numpy(plan).cuda(), torch.from_numpy(clips).cuda(), torch.from_numpy(rat).cuda()
    lib = L.lib()
    ms_masked, _ = _timed(lambda: L.check(lib.sos_window_stage_masked_f32(L.ptr(flat), L.ptr(d_bits), L.ptr(d_clips), clips.ctypes.data,
                                                                          L.ptr(d_rat), rat.ctypes.data, len(ns), L.ptr(d_plan),
                                                                          plan.ctypes.data, W, stride, L.ptr(wave), L.ptr(masked),
                                                                          L.stream_ptr())), 200)
    ms_plain, _ = _timed(lambda: L.check(lib.sos_window_stage_f32(L.ptr(flat), flat.numel(), L.ptr(d_plan), plan.ctypes.data, W, stride,
                                                                  L.ptr(wave), L.stream_ptr())), 200)
    frames = [len(b) for b in bits]
    rates = [30.0] * len(ns)
    wf = np.asarray(windows._window_frames(plan, SR, rates, frames), dtype=np.int64)
    first = windows._first_windows(plan, len(ns))
    recs = np.ascontiguousarray(np.stack([ragged.offsets(frames), np.asarray(frames, dtype=np.int64), first[:-1], np.diff(first)], axis=1))
    logit_rows = torch.randn((W, int(wf.max())), device="cuda")
    out = tools.window_frames_stitch(logit_rows, plan, wf, recs, rat, core, context)
    d_wf, d_recs = torch.from_numpy(wf).cuda(), torch.from_numpy(recs).cuda()
    ms_frames, _ = _timed(lambda: L.check(lib.sos_window_frames_stitch_f32(L.ptr(logit_rows), W, logit_rows.shape[1], L.ptr(d_plan),
                                                                           plan.ctypes.data, L.ptr(d_wf), wf.ctypes.data, W,
                                                                           L.ptr(d_recs), recs.ctypes.data, L.ptr(d_rat), rat.ctypes.data,
                                                                           len(ns), core, context, L.ptr(out), L.stream_ptr())), 200)
    for name, ms, floats in (("sos_window_stage_masked_f32", ms_masked, int(plan[:, 2].sum()) + 2 * wave.numel()),
                             ("sos_window_stage_f32 (the same windows, wave rows only)", ms_plain, int(plan[:, 2].sum()) + wave.numel()),
                             ("sos_window_frames_stitch_f32", ms_frames, 2 * out.numel())):
        src, dst = torch.empty(max(floats // 2, 1), device="cuda"), torch.empty(max(floats // 2, 1), device="cuda")
        ms_copy, _ = _timed(lambda: dst.copy_(src), 200)
        nbytes = 4.0 * floats
        print(f"{name} ({W} windows of {len(ns)} recordings, resident buffers): {ms * 1e3:8.1f} us, {nbytes / 1e6:.2f} MB at "
              f"{nbytes / (ms / 1e3) / 1e12:.3f} TB/s; a float4 copy of the same bytes {ms_copy * 1e3:8.1f} us "
              f"({nbytes / (ms_copy / 1e3) / 1e12:.3f} TB/s)")


def signals(args, det, jm):
    from sos_amd import ragged
    n = int(args.seconds * SR)
    mixed = [_wave(800, n)] + [_wave(801 + i, 2 * SR) for i in range(63)]
    rng = np.random.default_rng(14)
    bits = [torch.from_numpy(rng.integers(0, 2, pipeline.n_video_frames(c.numel())).astype(np.uint8)).cuda() for c in mixed]
    kw = dict(window_seconds=30.0, context_seconds=args.context)
    if not args.kernels_only:
        sos_amd.set_precision(args.precision)
        try:
            for name, fn in (("bits= path, the output alone", lambda: pipeline.denoise_long(None, jm, mixed, bits=bits, fps=30.0, **kw)),
                             ("bits= path, signals=True (four signals)", lambda: pipeline.denoise_long(None, jm, mixed, bits=bits, fps=30.0, signals=True, **kw))):
                ms, peak = _timed(fn, args.iters)
                print(f"{args.seconds:g} s + 63 x 2 s at {SR} Hz, {args.precision}, 30 s windows: {name} {ms:9.1f} ms per call, peak {peak / 2**30:6.2f} GiB")
        finally:
            sos_amd.set_precision("bf16")
    # the kernels alone, on resident buffers: the mixed batch's plan, four planes of random rows
    hop, planes = transform.HOP_LENGTH, 4
    ns = [int(c.numel()) for c in mixed]
    core, context = windows._hops(round(30.0 * SR)), windows._hops(round(args.context * SR))
    held = np.ascontiguousarray(pipeline.window_plan(ns, core, context))
    held[:, 2] = hop * (held[:, 2] // hop)                      # what a window's row holds
    W, stride = len(held), int(held[:, 2].max())
    lens = [hop * (m // hop) for m in ns]
    total = sum(lens)
    rows = torch.randn((planes, W, stride), device="cuda")
    d_held = torch.from_numpy(held).cuda()
    lib = L.lib()

    def layout(pitch):
        recs = np.ascontiguousarray(np.stack([planes * ragged.offsets(pitch), np.asarray(pitch, dtype=np.int64)], axis=1))
        return recs, torch.from_numpy(recs).cuda(), torch.empty(planes * sum(pitch), device="cuda")

    def one_launch(recs, d_recs, out):
        return lambda: L.check(lib.sos_window_stitch_planes_f32(L.ptr(rows), planes, W, stride, L.ptr(d_held), held.ctypes.data, W,
                                                                context, L.ptr(d_recs), recs.ctypes.data, len(ns), out.numel(),
                                                                L.ptr(out), L.stream_ptr()))

    aligned, odd = one_launch(*layout([-(-m // 4) * 4 for m in lens])), one_launch(*layout(lens))
    # the sequence: one stitch per plane into a plane-major buffer, then one unpack launch over every output sample (its table
    # takes whole rows, so the four planes are its four rows: the bytes of the reordering, not the reordering itself)
    major, flat = torch.empty((planes, total), device="cuda"), torch.empty(planes * total, device="cuda")
    utab = np.ascontiguousarray(np.asarray([(q, total, q * total) for q in range(planes)], dtype=np.int64))
    d_utab = torch.from_numpy(utab).cuda()

    def sequence():
        for q in range(planes):
            L.check(lib.sos_window_stitch_f32(L.ptr(rows[q]), W, stride, L.ptr(d_held), held.ctypes.data, W, context, L.ptr(major[q]),
                                              L.stream_ptr()))
        L.check(lib.sos_ragged_unpack_f32(L.ptr(major), planes, total, L.ptr(d_utab), utab.ctypes.data, planes, L.ptr(flat), L.stream_ptr()))

    floats = planes * (2 * total + 2 * context * (W - len(ns)))
    src, dst = torch.empty(floats // 2, device="cuda"), torch.empty(floats // 2, device="cuda")
    runs = []
    for _ in range(args.signal_runs):                           # the two alternate
        runs.append((_timed(aligned, 200)[0], _timed(sequence, 200)[0], _timed(lambda: dst.copy_(src), 200)[0], _timed(odd, 200)[0]))
    nbytes = 4.0 * floats
    for i, (a, b, c, d) in enumerate(runs):
        print(f"run {i}: sos_window_stitch_planes_f32 ({planes} planes, {W} windows of {len(ns)} recordings, file-major) {a * 1e3:8.1f} us "
              f"({nbytes / 1e6:.1f} MB at {nbytes / (a / 1e3) / 1e12:.3f} TB/s); {planes} x sos_window_stitch_f32 + sos_ragged_unpack_f32 "
              f"{b * 1e3:8.1f} us; ratio {b / a:.2f}; a float4 copy of the one launch's bytes {c * 1e3:8.1f} us; file-major with "
              f"pitch = length (segments off 16-byte boundaries) {d * 1e3:8.1f} us")
    one, seq = [r[0] for r in runs], [r[1] for r in runs]
    spread = max(max(one) - min(one), max(seq) - min(seq))
    print(f"{len(runs)} alternating runs: one launch {np.median(one) * 1e3:.1f} us (min {min(one) * 1e3:.1f}, max {max(one) * 1e3:.1f}), the "
          f"sequence {np.median(seq) * 1e3:.1f} us (min {min(seq) * 1e3:.1f}, max {max(seq) * 1e3:.1f}), ratio of the medians "
          f"{np.median(seq) / np.median(one):.2f}; slowest one launch {'below' if max(one) + spread < min(seq) else 'NOT below'} the "
          f"fastest sequence by more than the spread between runs ({spread * 1e3:.1f} us)")


def distance(args, det, jm):
    n = 60 * SR
    clip = _wave(810, n)
    sos_amd.set_precision("bf16x3")
    try:
        whole = pipeline.denoise_ragged(det, jm, [clip])[0]
        scale = float(whole.abs().max())
        for win in args.distance_windows:
            for ctx in (0.0, 1.0, 2.0):
                got, extra = pipeline.denoise_long(det, jm, [clip], window_seconds=win, context_seconds=ctx, return_all=True)
                cores = [float((got[0][cs:ce] - whole[cs:ce]).abs().max()) / scale for cs, ce in extra[0]["plan"][:, 4:6].tolist()]
                rms = float(((got[0] - whole) ** 2).mean().sqrt() / (whole ** 2).mean().sqrt())
                print(f"60 s, bf16x3, closed-form networks: {win:g} s windows, context {ctx:g} s ({len(cores)} windows): max relative "
                      f"error over the cores {max(cores):.3e} (per core " + " ".join(f"{c:.1e}" for c in cores) + f"), rms relative {rms:.3e}")
    finally:
        sos_amd.set_precision("bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--windows", type=float, nargs="*", default=[10.0, 30.0, 60.0])
    ap.add_argument("--max-columns", type=int, nargs="*", default=[16384, 4096],
                    help="further runs at 30 s windows with these column budgets per group (the default budget is 65536)")
    ap.add_argument("--context", type=float, default=2.0)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--skip-whole", action="store_true", help="do not time the whole-file call")
    ap.add_argument("--distance", action="store_true", help="also report the distance from the whole-file result (60 s, bf16x3)")
    ap.add_argument("--distance-windows", type=float, nargs="*", default=[10.0, 30.0])
    ap.add_argument("--no-speed", action="store_true")
    ap.add_argument("--decisions", action="store_true", help="stitch_bits=True, the bits= path on a mixed batch, the two kernels alone")
    ap.add_argument("--kernels-only", action="store_true", help="with --decisions: only the kernels' lines")
    ap.add_argument("--signals", action="store_true", help="the planes stitch against four stitches and an unpack; signals=True")
    ap.add_argument("--signal-runs", type=int, default=3, help="with --signals: alternating runs of the one launch and the sequence")
    ap.add_argument("--root", default=None, help="measure another checkout of the repository (package and built libraries)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_bench needs an MI355X: nothing is measured without one")
    det, jm = _nets()
    with torch.no_grad():
        if not args.no_speed:
            speed(args, det, jm)
        if args.decisions:
            decisions(args, det, jm)
        if args.signals:
            signals(args, det, jm)
        if args.distance:
            distance(args, det, jm)


if __name__ == "__main__":
    main()
