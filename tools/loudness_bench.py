"""Loudness benchmark (run on the GPU box), 'mixed' precision, the files of tools/recordings_bench.py (N stereo 16-bit recordings
of 1 .. 10 s at 44.1 kHz, seeded):
  1. recordings.denoise_recordings(loudness=-23) against loudness=None on the same files, both warmed, alternating, --repeats
     times each: median wall time from an idle device to an idle device (file reads and writes included), spread, host waits.
  2. the measure sequence (sos_loudness_batch_f64: four launches) and the gain launch (sos_loudness_gain_batch_f32) alone, from
     device events over --kernel-reps calls, --kernel-repeats times per row, on the planes of those files and on --kernel-mib
     MiB of planes (stereo files of 2^20 frames), next to Tensor.copy_ moving the bytes each must move at the least: the measure
     sequence reads the planes twice (8 bytes per sample, counted as a copy of 4), the gain reads and writes them once.  Each
     twice: the Python call (table, coefficients and weights built and uploaded per call) and the C entry point with all of
     that already on the device; the entry point's rows are checked to be the Python call's.
  3. --true-peak: the other EBU R128 measures instead of 1. and 2., every row of a table measured once per round, --kernel-repeats
     alternating rounds: sos_true_peak_batch_f64 (the Python call and the entry point) on the files' planes and on --kernel-mib
     MiB of planes, next to Tensor.copy_ of the same bytes and to the way the number could be had before -- every channel
     through resample_batch_device to four times the rate, then abs().amax() per file (a torch conv1d with the true-peak
     coefficients where the resampler refuses the pair); sos_loudness_range_batch_f64 next to the measure sequence it follows;
     and denoise_recordings(loudness=-23, peak='true', loudness_range=True) against peak='sample', alternating.
  4. --limiter: the look-ahead limiter instead of 1. and 2., every row once per round, --kernel-repeats alternating rounds:
     sos_limiter_batch_f32 (the entry point with everything on the device, and the Python call) on the files' planes and on
     --kernel-mib MiB of planes -- with a target that leaves every sample under the ceiling (a tile then skips from the envelope
     to the store) and with one 15 dB up, where the peaks are 2.8 times over it, in the sample and the true-peak form -- next to
     Tensor.copy_ of the same bytes and to the same rule composed from torch ops per file (a channel amax, -max_pool1d(-r),
     avg_pool1d in float64), what a user would write without the kernel; and denoise_recordings(loudness=-16,
     limiter='lookahead') against limiter=None, alternating, with the count of peak_limited files and the mean |loudness -
     target| of either.  The files are SYNTHETIC (tools/recordings_bench.py): real speech has another crest factor.
A measurement: no time is asserted; the entry points' results are checked to be the Python calls' before they are timed."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recordings_bench as RB  # noqa: E402
import sos_amd  # noqa: E402
from oracle import nets as onet  # noqa: E402
from sos_amd import _lib as L, audio_io, metrics, ragged, recordings  # noqa: E402
from sos_amd.common import MyConfig  # noqa: E402
from sos_amd.denoiser import networks as jnet  # noqa: E402
from sos_amd.detector import networks as dnet  # noqa: E402


def launches(name, planes, rate, args):
    samples = sum(p.numel() for p in planes)
    rates = [rate] * len(planes)
    stats = metrics.loudness_batch(planes, rates)
    unit = torch.zeros(len(planes), dtype=torch.float64, device="cuda")                 # target = L: g = 1, the planes keep their level
    rows = []
    for split in args.splits:
        go = lambda: metrics.loudness_batch(planes, rates, split=split)                  # noqa: E731
        rows.append(("measure, split %d" % split, [RB.device_ms(go, args.kernel_reps) for _ in range(args.kernel_repeats)]))
    go = lambda: audio_io.loudness_gain_batch_device(planes, stats["rows"], stats["lufs"].contiguous() + unit, 0.0)   # noqa: E731
    rows.append(("gain", [RB.device_ms(go, args.kernel_reps) for _ in range(args.kernel_repeats)]))
    # the entry points themselves: table, coefficients, weights and work buffer already on the device
    h = L.lib()
    flat = ragged.back_to_back(planes)
    chans, avail = [p.shape[0] for p in planes], [p.shape[1] for p in planes]
    coef = torch.from_numpy(np.stack([metrics.k_weighting(rate)] * len(planes))).cuda()
    w = torch.ones(sum(chans), dtype=torch.float64, device="cuda")
    out = torch.empty((len(planes), 4), dtype=torch.float64, device="cuda")
    for split in args.splits:
        tab = metrics.loudness_table(chans, avail, avail, [metrics.loudness_hop(rate)] * len(planes), split)
        tab_dev = torch.from_numpy(tab).cuda()
        ws = torch.empty(h.sos_loudness_workspace_bytes(tab.ctypes.data_as(L.C.c_void_p), len(planes), split), dtype=torch.uint8, device="cuda")
        go = lambda: L.check(h.sos_loudness_batch_f64(L.ptr(flat), L.ptr(tab_dev), tab.ctypes.data_as(L.C.c_void_p), len(planes), L.ptr(coef),   # noqa: E731
                                                      L.ptr(w), split, L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()))
        rows.append(("  entry, split %d" % split, [RB.device_ms(go, args.kernel_reps) for _ in range(args.kernel_repeats)]))
        assert torch.equal(out, metrics.loudness_batch(planes, rates, split=split)["rows"])
    gains = torch.empty(len(planes), dtype=torch.float32, device="cuda")
    flags = torch.empty(len(planes), dtype=torch.int32, device="cuda")
    targets = stats["lufs"].contiguous() + unit
    go = lambda: L.check(h.sos_loudness_gain_batch_f32(L.ptr(flat), L.ptr(tab_dev), tab.ctypes.data_as(L.C.c_void_p), len(planes),          # noqa: E731
                                                       L.ptr(stats["rows"]), L.ptr(targets), 0.0, L.ptr(gains), L.ptr(flags), L.stream_ptr()))
    rows.append(("  entry, gain", [RB.device_ms(go, args.kernel_reps) for _ in range(args.kernel_repeats)]))
    src = torch.empty(samples, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    copy = [RB.device_ms(lambda: dst.copy_(src), args.kernel_reps) for _ in range(args.kernel_repeats)]
    copy_ms = float(np.median(copy))
    print(f"{name}: {len(planes)} files, {samples * 4 / 2**20:.1f} MiB of planes, {args.kernel_reps} calls per measurement, "
          f"{args.kernel_repeats} measurements per row (median, min, max); 'measure' / 'gain' are the Python calls with their "
          "table uploads, 'entry' rows the C entry points with everything already on the device")
    print(f"  Tensor.copy_ of the planes (one read, one write): {copy_ms:8.3f} ms (min {min(copy):.3f}, max {max(copy):.3f})  "
          f"{samples * 8 / copy_ms / 1e6:7.1f} GB/s")
    for what, runs in rows:
        ms = float(np.median(runs))
        print(f"  {what:17s}: {ms:8.3f} ms (min {min(runs):.3f}, max {max(runs):.3f})  {samples * 8 / ms / 1e6:7.1f} GB/s of the 8 bytes per "
              f"sample it must move   {ms / copy_ms:6.2f} x the copy")


def _rounds(rows, args):
    """{name: [ms, ..]}: every row once per round, the rows alternating."""
    runs = {name: [] for name, _, _ in rows}
    for _ in range(args.kernel_repeats):
        for name, fn, reps in rows:
            runs[name].append(RB.device_ms(fn, reps))
    return runs


def _oversampled_peaks(planes, rate):
    """The true peak as it could be had without the kernel: (what ran, a function returning one peak per file)."""
    channels = [p[c] for p in planes for c in range(p.shape[0])]
    owner = torch.tensor([i for i, p in enumerate(planes) for _ in range(p.shape[0])], device="cuda")

    def per_file(peaks):
        return torch.zeros(len(planes), device="cuda").index_reduce_(0, owner, peaks, "amax", include_self=True)

    def resampled():
        up = audio_io.resample_batch_device(channels, rate, 4 * rate)
        return per_file(torch.stack([u.abs().amax() for u in up]))

    try:
        resampled()
        return "resample_batch_device to 4x, abs().amax()", resampled
    except (ValueError, RuntimeError) as e:
        print("  resample_batch_device(%d -> %d) refused (%s): torch conv1d with the true-peak coefficients instead" % (rate, 4 * rate, e))
    coef = torch.from_numpy(metrics.true_peak_filter()).cuda().flip(1).unsqueeze(1)      # conv1d correlates: taps reversed

    def convolved():
        peaks = [torch.maximum(torch.nn.functional.conv1d(c.view(1, 1, -1), coef, padding=6).abs().amax(), c.abs().amax()) for c in channels]
        return per_file(torch.stack(peaks))
    return "torch conv1d with the coefficients, abs().amax()", convolved


def true_peak_launches(name, planes, rate, args):
    samples = sum(p.numel() for p in planes)
    h = L.lib()
    flat = ragged.back_to_back(planes)
    chans, avail = [p.shape[0] for p in planes], [p.shape[1] for p in planes]
    split = metrics.LOUDNESS_SPLIT
    tab = metrics.loudness_table(chans, avail, avail, [metrics.loudness_hop(rate)] * len(planes), split)
    tab_dev, host = torch.from_numpy(tab).cuda(), tab.ctypes.data_as(L.C.c_void_p)
    tp_coef = torch.from_numpy(metrics.true_peak_filter()).cuda()
    peaks = torch.empty(len(planes), dtype=torch.float64, device="cuda")
    coef = torch.from_numpy(np.stack([metrics.k_weighting(rate)] * len(planes))).cuda()
    w = torch.ones(sum(chans), dtype=torch.float64, device="cuda")
    rows4, out4 = (torch.empty((len(planes), 4), dtype=torch.float64, device="cuda") for _ in range(2))
    ws = torch.empty(h.sos_loudness_workspace_bytes(host, len(planes), split), dtype=torch.uint8, device="cuda")
    rw = torch.empty(h.sos_loudness_range_workspace_bytes(host, len(planes)), dtype=torch.uint8, device="cuda")
    src = torch.empty(samples, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    entry = lambda: L.check(h.sos_true_peak_batch_f64(L.ptr(flat), L.ptr(tab_dev), host, len(planes), L.ptr(tp_coef), L.ptr(peaks),   # noqa: E731
                                                      L.stream_ptr()))
    measure = lambda: L.check(h.sos_loudness_batch_f64(L.ptr(flat), L.ptr(tab_dev), host, len(planes), L.ptr(coef), L.ptr(w), split,  # noqa: E731
                                                       L.ptr(ws), ws.numel(), L.ptr(rows4), L.stream_ptr()))
    ranges = lambda: L.check(h.sos_loudness_range_batch_f64(L.ptr(tab_dev), host, len(planes), L.ptr(w), split, L.ptr(ws), ws.numel(),  # noqa: E731
                                                            L.ptr(rw), rw.numel(), L.ptr(out4), L.stream_ptr()))
    how, before = _oversampled_peaks(planes, rate)
    entry()
    old = before().double()
    print(f"{name}: {len(planes)} files, {samples * 4 / 2**20:.1f} MiB of planes; largest relative difference of the kernel's peaks from "
          f"'{how}': {float(((peaks - old).abs() / peaks.clamp_min(1e-30)).max()):.2e}")
    assert torch.equal(peaks, metrics.true_peak_batch(planes))
    measure()
    rows = [("Tensor.copy_ of the planes", lambda: dst.copy_(src), args.kernel_reps),
            ("true peak, entry point", entry, args.kernel_reps),
            ("true peak, Python call", lambda: metrics.true_peak_batch(planes), args.kernel_reps),
            (how, before, 1),
            ("measure sequence, entry", measure, args.kernel_reps),
            ("range sequence, entry", ranges, args.kernel_reps)]
    runs = _rounds(rows, args)
    copy_ms = float(np.median(runs[rows[0][0]]))
    print(f"  {args.kernel_repeats} alternating rounds, {args.kernel_reps} calls per measurement (1 for the old way): median (min, max)")
    for what, _, _ in rows:
        ms = float(np.median(runs[what]))
        print(f"  {what:46s}: {ms:9.3f} ms (min {min(runs[what]):.3f}, max {max(runs[what]):.3f})  {samples * 4 / ms / 1e6:8.1f} GB/s of "
              f"plane bytes read   {samples * 36 / ms / 1e9:7.2f} TFMA/s if it were the kernel   {ms / copy_ms:7.2f} x the copy")


def true_peak_calls(paths, tmp, secs, args):
    det = dnet.get_network()
    det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    det, jm = det.cuda().eval(), jm.cuda().eval()
    sos_amd.set_precision("mixed")
    forms = dict(sample=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "sample"), max_batch=args.max_batch,
                                                              loudness=args.target, peak="sample"),
                 true=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "true"), max_batch=args.max_batch,
                                                            loudness=args.target, peak="true", loudness_range=True))
    for fn in forms.values():
        fn()
    runs = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, fn in forms.items():
            runs[k].append(RB.once(fn))
    print(f"{args.files} stereo s16 files at {RB.RATE} Hz, {secs:.0f} s of audio x 2 channels, 'mixed' precision, {args.repeats} "
          "alternating repeats (median, min, max)")
    a = RB.report("peak='sample'", args.files, runs["sample"])
    b = RB.report("peak='true', loudness_range", args.files, runs["true"])
    print(f"  true peak and range / sample peak = {b / a:.3f}")
    sos_amd.set_precision("bf16")


def _torch_limit(planes, s, ceiling, H):
    """The sample form of the rule from torch ops, file by file."""
    F = torch.nn.functional
    outs = []
    for x, sf in zip(planes, s):
        a = x.abs().amax(dim=0) * sf
        r = torch.where(a > ceiling, (ceiling / a).clamp_min(2.0 ** -10), torch.ones_like(a))
        mn = -F.max_pool1d(-F.pad(r.view(1, 1, -1), (2 * H, 2 * H), value=1.0), 2 * H + 1, 1)
        g = F.avg_pool1d(mn.double(), 2 * H + 1, 1).float().view(-1)
        outs.append(x * (g * sf))
    return outs


def limiter_launches(name, planes, rate, args):
    samples = sum(p.numel() for p in planes)
    h = L.lib()
    H = audio_io.limiter_lookahead("loudness_bench", rate, args.lookahead_ms, len(planes))[0]
    flat = ragged.back_to_back(planes)
    out = torch.empty_like(flat)
    chans, avail = [p.shape[0] for p in planes], [p.shape[1] for p in planes]
    tab = metrics.loudness_table(chans, avail, avail, [metrics.loudness_hop(rate)] * len(planes), 1)
    tab[:, 4] = H
    tab_dev, host = torch.from_numpy(tab).cuda(), tab.ctypes.data_as(L.C.c_void_p)
    coef = torch.from_numpy(metrics.true_peak_filter()).cuda()
    stats = metrics.loudness_batch(planes, [rate] * len(planes))
    ceiling = float(np.float32(10.0 ** (args.ceiling / 20.0)))
    peak = stats["peak"].clamp_min(1e-30)
    under = (stats["lufs"] + 20.0 * torch.log10(0.5 * ceiling / peak)).contiguous()           # s * peak = 0.5 C: no sample or point over
    over = (under + 15.0).contiguous()                                                        # s * peak = 2.8 C
    rows4 = torch.empty((len(planes), 4), dtype=torch.float64, device="cuda")
    entry = lambda t, tp: L.check(h.sos_limiter_batch_f32(L.ptr(flat), L.ptr(out), L.ptr(tab_dev), host, len(planes), L.ptr(stats["rows"]),  # noqa: E731
                                                          L.ptr(t), args.ceiling, tp, L.ptr(coef), L.ptr(rows4), L.stream_ptr()))
    call = lambda t, tp=False: audio_io.limit_batch_device(planes, stats["rows"], t, args.ceiling, rates=rate,  # noqa: E731
                                                          lookahead_ms=args.lookahead_ms, true_peak=tp)
    limited, curve = call(over)
    entry(over, 0)
    assert torch.equal(out, ragged.back_to_back(limited)) and torch.equal(rows4, curve)
    s = curve[:, 0].float()
    old = _torch_limit(planes, s, ceiling, H)
    worst = max(float((a - b).abs().max()) for a, b in zip(old, limited))
    share = float(curve[:, 2].sum()) * sum(chans) / len(planes) / samples
    print(f"{name}: {len(planes)} files, {samples * 4 / 2**20:.1f} MiB of planes, H = {H} samples ({args.lookahead_ms} ms at {rate} Hz), "
          f"ceiling {args.ceiling} dB; 15 dB up: least g {float(curve[:, 1].min()):.3f}, {100 * share:.1f} % of the samples lowered; largest "
          f"|kernel - torch ops| {worst:.2e}")
    src = torch.empty(samples, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    rows = [("Tensor.copy_ of the planes", lambda: dst.copy_(src), args.kernel_reps),
            ("entry, sample form, no sample over", lambda: entry(under, 0), args.kernel_reps),
            ("entry, sample form, 15 dB up", lambda: entry(over, 0), args.kernel_reps),
            ("entry, true-peak form, no sample over", lambda: entry(under, 1), args.kernel_reps),
            ("entry, true-peak form, 15 dB up", lambda: entry(over, 1), args.kernel_reps),
            ("Python call, sample form, 15 dB up", lambda: call(over), args.kernel_reps),
            ("torch ops per file, sample form", lambda: _torch_limit(planes, s, ceiling, H), 1)]
    runs = _rounds(rows, args)
    copy_ms = float(np.median(runs[rows[0][0]]))
    print(f"  {args.kernel_repeats} alternating rounds, {args.kernel_reps} calls per measurement (1 for the torch ops): median (min, max)")
    for what, _, _ in rows:
        ms = float(np.median(runs[what]))
        print(f"  {what:42s}: {ms:9.3f} ms (min {min(runs[what]):.3f}, max {max(runs[what]):.3f})  {samples * 8 / ms / 1e6:8.1f} GB/s of the 8 bytes "
              f"per sample a copy moves   {ms / copy_ms:7.2f} x the copy")


def limiter_calls(paths, tmp, secs, args):
    det = dnet.get_network()
    det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    det, jm = det.cuda().eval(), jm.cuda().eval()
    sos_amd.set_precision("mixed")
    kw = dict(max_batch=args.max_batch, loudness=args.limiter_target, peak_ceiling_db=args.ceiling)
    forms = dict(none=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "none"), **kw),
                 lookahead=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "lookahead"), limiter="lookahead",
                                                                 lookahead_ms=args.lookahead_ms, **kw))
    res = {k: fn() for k, fn in forms.items()}                                            # the warm-up, and the rows
    runs = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, fn in forms.items():
            runs[k].append(RB.once(fn))
    print(f"{args.files} SYNTHETIC stereo s16 files at {RB.RATE} Hz, {secs:.0f} s of audio x 2 channels, 'mixed' precision, loudness="
          f"{args.limiter_target}, ceiling {args.ceiling} dB, {args.repeats} alternating repeats (median, min, max)")
    a = RB.report("limiter=None", args.files, runs["none"])
    b = RB.report("limiter='lookahead'", args.files, runs["lookahead"])
    print(f"  with the limiter / without = {b / a:.3f}")
    for k, rows in res.items():
        miss = [abs(r["loudness"] - r["loudness_target"]) for r in rows]
        print(f"  {k:9s}: {sum(r['peak_limited'] for r in rows)} of {len(rows)} files peak_limited, mean |loudness - target| {np.mean(miss):.4f} LU "
              f"(largest {max(miss):.4f})" + ("" if k == "none" else f", {sum(r['limiter_samples'] > 0 for r in rows)} files with a lowered "
                                              f"sample, least limiter_db {min(r['limiter_db'] for r in rows):.2f}"))
    sos_amd.set_precision("bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--target", type=float, default=-23.0)
    ap.add_argument("--kernel-mib", type=int, default=512)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--kernel-repeats", type=int, default=3)
    ap.add_argument("--splits", type=int, nargs="+", default=[metrics.LOUDNESS_SPLIT])
    ap.add_argument("--skip-calls", action="store_true", help="only the launches")
    ap.add_argument("--true-peak", action="store_true", help="the true-peak and loudness-range rows instead of the others")
    ap.add_argument("--limiter", action="store_true", help="the look-ahead limiter's rows instead of the others")
    ap.add_argument("--limiter-target", type=float, default=-16.0, help="--limiter: the loudness target of the denoise_recordings calls")
    ap.add_argument("--ceiling", type=float, default=-1.0, help="--limiter: the peak ceiling in dB")
    ap.add_argument("--lookahead-ms", type=float, default=5.0)
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    RB._count_downloads()
    with tempfile.TemporaryDirectory() as tmp:
        paths, secs = RB.make_files(tmp, args.files, args.seed)
        if args.limiter:
            if not args.skip_calls:
                limiter_calls(paths, tmp, secs, args)
            ys, _, _ = audio_io.load_channels_batch_device(paths, sr=None)
            limiter_launches("the files' planes", ys, RB.RATE, args)
        elif args.true_peak:
            if not args.skip_calls:
                true_peak_calls(paths, tmp, secs, args)
            ys, _, _ = audio_io.load_channels_batch_device(paths, sr=None)
            true_peak_launches("the files' planes", ys, RB.RATE, args)
        elif not args.skip_calls:
            det = dnet.get_network()
            det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
            jm = jnet.get_network(MyConfig())
            jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
            det, jm = det.cuda().eval(), jm.cuda().eval()
            sos_amd.set_precision("mixed")
            forms = dict(none=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "none"), max_batch=args.max_batch),
                         level=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "level"), max_batch=args.max_batch,
                                                                     loudness=args.target))
            for fn in forms.values():                                                     # warm-up of both forms
                fn()
            runs = {k: [] for k in forms}
            for _ in range(args.repeats):                                                 # the forms alternate
                for k, fn in forms.items():
                    runs[k].append(RB.once(fn))
            print(f"{args.files} stereo s16 files at {RB.RATE} Hz, {secs:.0f} s of audio x 2 channels, 'mixed' precision, {args.repeats} "
                  "alternating repeats (median, min, max)")
            a = RB.report("loudness=None", args.files, runs["none"])
            b = RB.report("loudness=%g" % args.target, args.files, runs["level"])
            print(f"  levelled / plain = {b / a:.3f}")
            sos_amd.set_precision("bf16")
        if not args.true_peak and not args.limiter:
            ys, _, _ = audio_io.load_channels_batch_device(paths, sr=None)
            launches("the files' planes", ys, RB.RATE, args)
    frames, ch = 1 << 20, 2
    n_files = max(1, (args.kernel_mib << 20) // (4 * frames * ch))
    flat = torch.empty(n_files * ch * frames, dtype=torch.float32, device="cuda").uniform_(-0.5, 0.5)
    (limiter_launches if args.limiter else true_peak_launches if args.true_peak else launches)("large planes", [v.view(ch, frames) for v in flat.split(ch * frames)], RB.RATE, args)


if __name__ == "__main__":
    main()
