"""Recordings benchmark (run on the GPU box): N synthetic recordings of 1 .. 10 s (seeded lengths, stereo 16-bit PCM at 44.1 kHz)
in a temporary directory, in 'mixed' precision:
  1. recordings.denoise_recordings (one group) against the loop it replaces -- per file and per channel: read_wave, decode,
     resample_device, denoise_long, resample_device back, download, numpy quantisation; then one write per file.  Both forms are
     warmed once, then alternate, --repeats times each; the median wall time from an idle device to an idle device (file reads
     and writes included), the spread, files/s and the number of host waits (Tensor.cpu calls) are printed.
  2. the share of a denoise_recordings call that is not denoise_long: the same channels, already decoded and at 14 kHz, through
     denoise_long alone, timed the same way.
  3. the two kernels of csrc/pcm_io.hip on --kernel-mib MiB of planes (stereo files of 2^20 frames), every linear format and
     both G.711 laws: bytes read plus bytes written per second, from device events over --kernel-reps launches, --kernel-repeats
     times per row, against Tensor.copy_ of a float32 buffer moving the same number of bytes in the same run; each law also as
     a ratio to the u8 row, which moves the same bytes through the same accesses; the encode once on planes that never
     saturate and once on planes of which 9 % do (every workgroup then adds to its file's count).
  4. with --link-channels any|mean: (a) denoise_recordings(link_channels=) against link_channels=None on the same files, both
     warmed, alternating, in the same run of the program -- the linked mode runs denoise_long(stitch_bits=True), a separate
     detector pass, so it is expected to cost more, and the figure is what the shared stream costs; (b) the ONE
     sos_window_frames_link_f32 launch against what it replaces -- one stitch launch, one torch reduction per file in a Python
     loop, one concatenation and one threshold launch -- on the same random logit rows of the same files' plan
     (--link-window-seconds long windows), wall time per call from an idle device to an idle device, --link-reps calls each,
     alternating.  Both forms are checked to give the same bits before they are timed.
  5. with --high-band keep|follow: (a) denoise_recordings(high_band=) against high_band='drop' on the same files, both warmed,
     alternating, in the same run of the program: what putting the band above 7 kHz back costs per call; (b) the ONE
     sos_resample_merge_batch_f32 launch (with gains under 'follow') against the composition it replaces -- two
     resample_batch_device launches and two torch elementwise ops -- on the same channels at 14 kHz (native planes of (int)(m * ratio)
     frames, so that the composition needs no per-clip fitting), --band-reps alternating calls each, wall time from an idle device to an
     idle device; both forms are checked to give the same bits under 'keep' before they are timed; (c) the merge and the gains
     launch from device events against Tensor.copy_ moving the bytes they read and write.
  6. with --dither tpdf|highpass: (a) denoise_recordings(dither=) against dither=None on the same files, both warmed, alternating,
     in the same run of the program; (b) sos_pcm_encode_dither_batch (both kinds) against sos_pcm_encode_batch for u8 / s16 / s24 on
     the --kernel-mib MiB of stereo planes of 3., the three forms of a format alternating, --kernel-repeats times each, from device
     events over --kernel-reps launches: times, the ratio to the undithered kernel and to Tensor.copy_ of the same bytes; the same
     once more on one-channel files (a thread's four frames then share a Philox block; a stereo thread's share two); (c) with
     --against-lib PATH (another build of libsos_hip.so, e.g. the parent commit's): the undithered rows of this build against
     that build's, alternating, each with its own repeat spread.
A measurement: nothing is asserted."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sos_amd  # noqa: E402
from oracle import nets as onet  # noqa: E402
from sos_amd import _lib, audio_io, pipeline, ragged, recordings, resampling, tools, transform, windows  # noqa: E402
from sos_amd.common import MyConfig  # noqa: E402
from sos_amd.denoiser import networks as jnet  # noqa: E402
from sos_amd.detector import networks as dnet  # noqa: E402

WAITS = [0]
RATE = 44100


def _count_downloads():
    orig = torch.Tensor.cpu

    def cpu(self, *a, **k):
        if self.is_cuda:
            WAITS[0] += 1
        return orig(self, *a, **k)
    torch.Tensor.cpu = cpu


def once(fn):
    """(wall seconds, host waits) of one call, from an idle device to an idle device."""
    torch.cuda.synchronize()
    WAITS[0] = 0
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, WAITS[0]


def make_files(root, n_files, seed):
    rng = np.random.default_rng(seed)
    paths, secs = [], 0.0
    for i in range(n_files):
        n = int(rng.integers(RATE, 10 * RATE + 1))
        t = np.arange(n) / RATE
        sig = np.stack([0.3 * (np.sin(2 * np.pi * 0.7 * t + i + c) > -0.2) * np.sin(2 * np.pi * (220 + 40 * c) * t)
                        + 0.05 * rng.standard_normal(n) for c in range(2)], axis=1)
        paths.append(os.path.join(root, "rec_%03d.wav" % i))
        with open(paths[-1], "wb") as fp:
            fp.write(audio_io.wave_bytes(np.rint(sig * 32767).clip(-32768, 32767).astype(np.int16), RATE))
        secs += n / RATE
    return paths, secs


def per_file_loop(det, jm, paths, out_dir):
    """What a caller had before denoise_recordings: every channel on its own through the mono pieces, quantised on the host."""
    os.makedirs(out_dir, exist_ok=True)
    for path in paths:
        arr, kind, rate = audio_io.read_wave(path)
        chans = []
        for c in range(arr.shape[1]):
            y = audio_io.pcm_to_mono_device(torch.from_numpy(np.ascontiguousarray(arr[:, c:c + 1])).cuda(), kind)
            y = audio_io.resample_device(y, rate, pipeline.SR)
            y = windows.denoise_long(det, jm, [y])[0]
            y = audio_io.resample_device(y, pipeline.SR, rate).cpu().numpy()
            x = np.zeros(arr.shape[0], dtype=np.float32)
            x[:min(len(y), len(x))] = y[:len(x)]
            chans.append(np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16))
        with open(os.path.join(out_dir, os.path.basename(path)), "wb") as fp:
            fp.write(audio_io.wave_bytes(np.stack(chans, axis=1), rate))


def report(name, n_files, runs):
    ts, waits = [r[0] for r in runs], [r[1] for r in runs]
    med = float(np.median(ts))
    print(f"  {name:26s}: {med * 1e3:9.1f} ms (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f})   {n_files / med:8.1f} files/s   "
          f"host waits {int(np.median(waits))}")
    return med


def device_ms(fn, reps):
    """Milliseconds per call from device events around `reps` calls, after one warm-up call."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernels(args, amplitude):
    frames, ch = 1 << 20, 2
    n_files = max(1, (args.kernel_mib << 20) // (4 * frames * ch))
    samples = n_files * ch * frames
    flat = torch.empty(samples, dtype=torch.float32, device="cuda").uniform_(-amplitude, amplitude)
    planes = [v.view(ch, frames) for v in flat.split(ch * frames)]
    print(f"kernels: {n_files} files of {ch} x {frames} frames = {samples * 4 / 2**20:.0f} MiB of planes uniform in +-{amplitude:g} "
          f"({100 * float((flat.abs() >= 1).float().mean()):.1f} % of the samples saturate), {args.kernel_reps} launches each (bytes read + "
          "bytes written per second; the entry points themselves, tables already on the device)")
    L = _lib
    rows = []
    assert torch.equal(audio_io.encode_batch_device(planes[:1], "f32")[0].view(torch.float32), planes[0].T.reshape(-1))
    for fmt in ("s16", "s24", "s32", "u8", "f32", "alaw", "ulaw"):               # G.711 moves u8's bytes through u8's accesses
        g711 = fmt in audio_io.G711
        code, width = (audio_io.G711 if g711 else audio_io.ENCODINGS)[fmt][:2]
        entry = L.lib().sos_g711_encode_batch if g711 else L.lib().sos_pcm_encode_batch
        tab = np.asarray([[i * ch * frames, frames, ch, frames, i * ch * frames] for i in range(n_files)], dtype=np.int64)
        tab_dev, out = torch.from_numpy(tab).cuda(), torch.empty(samples * width, dtype=torch.uint8, device="cuda")
        counts = torch.empty(n_files, dtype=torch.int64, device="cuda")
        go = lambda: L.check(entry(L.ptr(flat), L.ptr(tab_dev), tab.ctypes.data_as(L.C.c_void_p), n_files, code, L.ptr(out),   # noqa: E731
                                   L.ptr(counts), L.stream_ptr()))
        rows.append(("encode " + fmt, samples * (4 + width), [device_ms(go, args.kernel_reps) for _ in range(args.kernel_repeats)]))
    for kind, dtype in (("s16", np.int16), ("s32", np.int32), ("u8", np.uint8), ("f32", np.float32), ("alaw", np.uint8),
                        ("ulaw", np.uint8)) if amplitude < 1 else ():
        g711 = kind in audio_io.G711
        code = audio_io.DECODE[kind][1]
        entry = L.lib().sos_g711_planes_batch_f32 if g711 else L.lib().sos_pcm_planes_batch_f32
        pcm = torch.zeros(samples, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
        tab = np.asarray([[i * ch * frames, frames, ch, i * ch * frames] for i in range(n_files)], dtype=np.int64)
        tab_dev, out = torch.from_numpy(tab).cuda(), torch.empty(samples, dtype=torch.float32, device="cuda")
        go = lambda: L.check(entry(L.ptr(pcm), code, L.ptr(tab_dev), tab.ctypes.data_as(L.C.c_void_p), n_files, L.ptr(out),     # noqa: E731
                                   L.stream_ptr()))
        rows.append(("decode " + kind, samples * (4 + dtype().itemsize), [device_ms(go, args.kernel_reps) for _ in range(args.kernel_repeats)]))
    med = {}
    for name, nbytes, runs in rows:
        src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        copy_ms = device_ms(lambda: dst.copy_(src), args.kernel_reps)
        ms = med[name] = float(np.median(runs))
        print(f"  {name:11s}: {ms:7.3f} ms (min {min(runs):.3f}, max {max(runs):.3f})  {nbytes / ms / 1e6:7.1f} GB/s    Tensor.copy_ of the "
              f"same bytes: {copy_ms:7.3f} ms  {nbytes / copy_ms / 1e6:7.1f} GB/s    ratio {copy_ms / ms:.2f}")
    for name, _, runs in rows:                                   # the yardstick of a law is u8 in the same run, with its spread
        way, fmt = name.split()
        if fmt in audio_io.G711:
            u8 = next(r for n, _, r in rows if n == way + " u8")
            print(f"  {name} / {way} u8 = {med[name] / med[way + ' u8']:.3f}   (u8 over its {len(u8)} repeats: "
                  f"{min(u8) / med[way + ' u8']:.3f} .. {max(u8) / med[way + ' u8']:.3f} of its median)")


def dither_kernels(args, ch, other=None):
    """6 (b), (c): per format the undithered entry point, the two dithered ones and, with `other`, another build's undithered one,
    alternating on the same planes."""
    L = _lib
    frames = (1 << 20) * 2 // ch
    n_files = max(1, (args.kernel_mib << 20) // (4 * frames * ch))
    samples = n_files * ch * frames
    flat = torch.empty(samples, dtype=torch.float32, device="cuda").uniform_(-0.9, 0.9)
    print(f"dither kernels: {n_files} files of {ch} x {frames} frames = {samples * 4 / 2**20:.0f} MiB of planes uniform in +-0.9, "
          f"{args.kernel_reps} launches per measurement, {args.kernel_repeats} measurements per form, the forms of a format alternating")
    base = np.asarray([[i * ch * frames, frames, ch, frames, i * ch * frames] for i in range(n_files)], dtype=np.int64)
    wide = np.ascontiguousarray(np.concatenate([base, np.arange(n_files, dtype=np.int64)[:, None], np.zeros((n_files, 1), np.int64)], axis=1))
    base_dev, wide_dev = torch.from_numpy(base).cuda(), torch.from_numpy(wide).cuda()
    counts = torch.empty(n_files, dtype=torch.int64, device="cuda")
    for fmt in audio_io.DITHER_FORMATS:
        code, width = audio_io.ENCODINGS[fmt][:2]
        out = torch.empty(samples * width, dtype=torch.uint8, device="cuda")

        def plain(h):
            return lambda: L.check(h.sos_pcm_encode_batch(L.ptr(flat), L.ptr(base_dev), base.ctypes.data_as(L.C.c_void_p), n_files, code,
                                                          L.ptr(out), L.ptr(counts), L.stream_ptr()))

        def dithered(kind):
            return lambda: L.check(L.lib().sos_pcm_encode_dither_batch(L.ptr(flat), L.ptr(wide_dev), wide.ctypes.data_as(L.C.c_void_p), n_files,
                                                                       code, audio_io.DITHER[kind], 1234, L.ptr(out), L.ptr(counts),
                                                                       L.stream_ptr()))

        forms = {"none": plain(L.lib()), "tpdf": dithered("tpdf"), "highpass": dithered("highpass")}
        if other is not None:
            forms["none, other build"] = plain(other)
        runs = {k: [] for k in forms}
        for r in range(args.kernel_repeats):                     # forwards, backwards, ..: no form always follows the same one
            for k, go in list(forms.items())[::-1 if r & 1 else 1]:
                runs[k].append(device_ms(go, args.kernel_reps))
        nbytes = samples * (4 + width)
        src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        copy_ms = device_ms(lambda: dst.copy_(src), args.kernel_reps)
        ref = float(np.median(runs["none"]))
        for k, r in runs.items():
            ms = float(np.median(r))
            print(f"  encode {fmt:3s} {k:17s}: {ms:7.3f} ms (min {min(r):.3f}, max {max(r):.3f})  {nbytes / ms / 1e6:7.1f} GB/s    / undithered "
                  f"{ms / ref:6.3f} (its repeats: {min(r) / ref:.3f} .. {max(r) / ref:.3f})    Tensor.copy_ of the same bytes {copy_ms:7.3f} ms, "
                  f"ratio {copy_ms / ms:.2f}")


def link_launch(args, paths):
    """4 (b): the link launch against stitch + per-file reduction + threshold on the same rows."""
    infos = [audio_io.wave_info(p) for p in paths]
    ns = [recordings._model_samples(i["frames"], i["rate"]) for i in infos for _ in range(i["channels"])]
    owner = [f for f, i in enumerate(infos) for _ in range(i["channels"])]
    core, context = windows._hops(round(args.link_window_seconds * pipeline.SR)), windows._hops(round(args.link_window_seconds / 8 * pipeline.SR))
    plan = windows.window_plan(ns, core, context)
    frames = [pipeline.n_video_frames(n) for n in ns]
    rates = [pipeline.FPS] * len(ns)
    wf = windows._window_frames(plan, pipeline.SR, rates, frames)
    first = windows._first_windows(plan, len(ns))
    recs = np.stack([ragged.offsets(frames), np.asarray(frames, dtype=np.int64), first[:-1], np.diff(first)], axis=1)
    links, members, _ = tools.link_tables(owner, frames)
    ratio = pipeline.SR / pipeline.FPS
    rows = torch.empty((len(plan), max(wf)), dtype=torch.float32, device="cuda").normal_()
    chans = [[int(m) for m in members[f:f + n]] for _, _, f, n in links]
    mode = args.link_channels

    def one():
        return tools.window_frames_link(rows, plan, wf, recs, ratio, core, context, links, members, mode, pipeline.SIGMOID_THRESHOLD)

    def pieces():
        per = ragged.split(tools.window_frames_stitch(rows, plan, wf, recs, ratio, core, context), frames)
        out = []
        for ch in chans:                                        # one reduction per file
            x = per[ch[0]]
            for m in ch[1:]:
                x = torch.maximum(x, per[m]) if mode == "any" else x + per[m]
            out.append(x / float(len(ch)) if mode == "mean" else x)
        logits = torch.cat(out)
        return logits, tools.threshold_bits(logits, pipeline.SIGMOID_THRESHOLD)[0]

    a, b = one(), pieces()
    same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    runs = dict(one=[], pieces=[])
    for _ in range(args.link_reps):
        runs["one"].append(once(one)[0])
        runs["pieces"].append(once(pieces)[0])
    t1, t2 = float(np.median(runs["one"])), float(np.median(runs["pieces"]))
    print(f"link launch: {len(links)} files, {len(ns)} channels, {len(plan)} windows of {args.link_window_seconds:g} s, {int(links[:, 1].sum())} "
          f"group frames, mode {mode}, {args.link_reps} alternating calls each (median wall time, idle device to idle device); "
          f"same logits and bits: {same}")
    print(f"  one sos_window_frames_link_f32 launch         : {t1 * 1e6:8.1f} us (min {min(runs['one']) * 1e6:.1f}, max {max(runs['one']) * 1e6:.1f})")
    print(f"  stitch + reduction per file + cat + threshold : {t2 * 1e6:8.1f} us (min {min(runs['pieces']) * 1e6:.1f}, max {max(runs['pieces']) * 1e6:.1f})"
          f"   ratio {t2 / t1:.2f}")


def band(args, paths):
    """5 (b), (c): the merge launch against two resamplings plus two elementwise ops, and both kernels against a copy."""
    ys, _, _ = audio_io.load_channels_batch_device(paths, sr=None)
    lows = audio_io.resample_batch_device([y[c] for y in ys for c in range(y.shape[0])], RATE, pipeline.SR)
    ratio = float(RATE) / pipeline.SR
    a = [t.clone() for t in lows]
    b = [0.5 * t for t in a]                                                     # m' = m: both resamplings have n = (int)(m * ratio) samples
    back = audio_io.resample_batch_device(a, pipeline.SR, RATE, fix=False)
    x_flat = ragged.back_to_back(back) + 0.01 * torch.randn(sum(t.numel() for t in back), device="cuda")   # native planes of that length
    xs = ragged.split(x_flat, [t.numel() for t in back])
    gains = audio_io.band_gains_batch_device(a, b) if args.high_band == "follow" else None

    def one():
        return audio_io.resample_merge_batch_device(xs, a, b, pipeline.SR, RATE, gains)

    def pieces():
        ra = audio_io.resample_batch_device(a, pipeline.SR, RATE, fix=False)
        rb = audio_io.resample_batch_device(b, pipeline.SR, RATE, fix=False)
        return torch.sub(x_flat, ragged.back_to_back(ra)).add_(ragged.back_to_back(rb))

    same = torch.equal(torch.cat(audio_io.resample_merge_batch_device(xs, a, b, pipeline.SR, RATE)), pieces())
    one(), pieces()
    runs = dict(one=[], pieces=[])
    for _ in range(args.band_reps):
        runs["one"].append(once(one)[0])
        runs["pieces"].append(once(pieces)[0])
    t1, t2 = float(np.median(runs["one"])), float(np.median(runs["pieces"]))
    n, m = sum(t.numel() for t in xs), sum(t.numel() for t in a)
    print(f"merge launch: {len(xs)} channels, {n} native frames at {RATE} Hz, {m} samples at {pipeline.SR} Hz, mode {args.high_band}, "
          f"{args.band_reps} alternating calls each (median wall time, idle device to idle device); keep gives the bits of the "
          f"composition: {same}")
    print(f"  one sos_resample_merge_batch_f32 launch       : {t1 * 1e6:8.1f} us (min {min(runs['one']) * 1e6:.1f}, max {max(runs['one']) * 1e6:.1f})")
    print(f"  two resample launches + sub + add             : {t2 * 1e6:8.1f} us (min {min(runs['pieces']) * 1e6:.1f}, max {max(runs['pieces']) * 1e6:.1f})"
          f"   ratio {t2 / t1:.2f}")
    # (c) the entry points themselves, tables already on the device, from device events
    L = _lib
    nn, mm = np.asarray([t.numel() for t in xs], dtype=np.int64), np.asarray([t.numel() for t in a], dtype=np.int64)
    J = -(-mm // transform.HOP_LENGTH)
    off = ragged.offsets
    tab = np.ascontiguousarray(np.stack([off(nn), nn, off(mm), mm, off(mm), mm, off(J), J, off(-(-nn // L.RESAMPLE_CHUNK))]), dtype=np.int64)
    gtab = np.ascontiguousarray(np.stack([off(mm), mm, off(mm), mm, off(J), J]), dtype=np.int64)
    tab_dev, gtab_dev = torch.from_numpy(tab).cuda(), torch.from_numpy(gtab).cuda()
    a_flat, b_flat = torch.cat(a), torch.cat(b)
    s_flat = torch.empty(int(J.sum()), dtype=torch.float32, device="cuda")
    out = torch.empty_like(x_flat)
    win, num_table = resampling.filter_on(x_flat.device, ratio, "kaiser_best")
    go_gain = lambda: L.check(L.lib().sos_band_gain_batch_f32(L.ptr(a_flat), L.ptr(b_flat), L.ptr(gtab_dev), gtab.ctypes.data_as(L.C.c_void_p),   # noqa: E731
                                                              len(xs), transform.HOP_LENGTH, 2, L.ptr(s_flat), L.stream_ptr()))
    go_merge = lambda s: L.check(L.lib().sos_resample_merge_batch_f32(L.ptr(x_flat), L.ptr(a_flat), L.ptr(b_flat), L.ptr(s), L.ptr(tab_dev),      # noqa: E731
                                                                      tab.ctypes.data_as(L.C.c_void_p), len(xs), ratio, L.ptr(win), win.numel(),
                                                                      num_table, transform.HOP_LENGTH, L.ptr(out), L.stream_ptr()))
    rows = [("gains", 4 * (2 * m + int(J.sum())), device_ms(go_gain, args.kernel_reps)),
            ("merge, g = 1", 4 * (2 * n + 2 * m), device_ms(lambda: go_merge(None), args.kernel_reps)),
            ("merge, gains", 4 * (2 * n + 2 * m + int(J.sum())), device_ms(lambda: go_merge(s_flat), args.kernel_reps))]
    for name, nbytes, ms in rows:
        src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        copy_ms = device_ms(lambda: dst.copy_(src), args.kernel_reps)
        print(f"  {name:13s}: {ms * 1e3:8.1f} us  {nbytes / ms / 1e6:7.1f} GB/s    Tensor.copy_ of the same bytes: {copy_ms * 1e3:8.1f} us  "
              f"{nbytes / copy_ms / 1e6:7.1f} GB/s    ratio {copy_ms / ms:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--kernel-mib", type=int, default=512)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--kernel-repeats", type=int, default=3, help="measurements per kernel row (median, min, max)")
    ap.add_argument("--amplitudes", type=float, nargs="+", default=[0.9, 1.1], help="encode inputs: nothing saturates below 1")
    ap.add_argument("--skip-loop", action="store_true", help="only the kernels")
    ap.add_argument("--link-channels", choices=["any", "mean"], default=None, help="measure the shared decision stream (4.) and nothing else")
    ap.add_argument("--link-window-seconds", type=float, default=2.0, help="4 (b): the windows of the link-launch comparison")
    ap.add_argument("--link-reps", type=int, default=50)
    ap.add_argument("--high-band", choices=["keep", "follow"], default=None, help="measure the merge of the band above 7 kHz (5.) and nothing else")
    ap.add_argument("--band-reps", type=int, default=30)
    ap.add_argument("--dither", choices=sorted(audio_io.DITHER), default=None, help="measure the dithered encode (6.) and nothing else")
    ap.add_argument("--against-lib", default=None, help="6 (c): another build of libsos_hip.so whose undithered encode is timed beside this one's")
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    _count_downloads()
    if args.dither:
        if not args.skip_loop:
            det = dnet.get_network()
            det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
            jm = jnet.get_network(MyConfig())
            jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
            det, jm = det.cuda().eval(), jm.cuda().eval()
            sos_amd.set_precision("mixed")
            with tempfile.TemporaryDirectory() as tmp:
                paths, secs = make_files(tmp, args.files, args.seed)
                forms = dict(plain=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "plain"), max_batch=args.max_batch),
                             dither=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "dither"), max_batch=args.max_batch,
                                                                          dither=args.dither, dither_seed=1234))
                for fn in forms.values():                                                 # warm-up of both forms
                    fn()
                runs = {k: [] for k in forms}
                for _ in range(args.repeats):                                             # the forms alternate
                    for k, fn in forms.items():
                        runs[k].append(once(fn))
                print(f"{args.files} stereo s16 files at {RATE} Hz, {secs:.0f} s of audio x 2 channels, 'mixed' precision, {args.repeats} "
                      "alternating repeats (median, min, max)")
                d = report("dither=None", args.files, runs["plain"])
                k = report("dither=%r" % args.dither, args.files, runs["dither"])
                print(f"  {args.dither} / none = {k / d:.3f}")
            sos_amd.set_precision("bf16")
        other = None
        if args.against_lib:
            other = _lib.C.CDLL(args.against_lib)
            other.sos_pcm_encode_batch.argtypes = _lib.SIGNATURES["sos_pcm_encode_batch"]
            print("other build:", args.against_lib)
        dither_kernels(args, 2, other)
        dither_kernels(args, 1, other)
        return
    if args.high_band:
        det = dnet.get_network()
        det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
        jm = jnet.get_network(MyConfig())
        jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
        det, jm = det.cuda().eval(), jm.cuda().eval()
        sos_amd.set_precision("mixed")
        with tempfile.TemporaryDirectory() as tmp:
            paths, secs = make_files(tmp, args.files, args.seed)
            forms = dict(drop=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "drop"), max_batch=args.max_batch),
                         band=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "band"), max_batch=args.max_batch,
                                                                    high_band=args.high_band))
            for fn in forms.values():                                                     # warm-up of both forms
                fn()
            runs = {k: [] for k in forms}
            for _ in range(args.repeats):                                                 # the forms alternate
                for k, fn in forms.items():
                    runs[k].append(once(fn))
            print(f"{args.files} stereo s16 files at {RATE} Hz, {secs:.0f} s of audio x 2 channels, 'mixed' precision, {args.repeats} "
                  "alternating repeats (median, min, max)")
            d = report("high_band='drop'", args.files, runs["drop"])
            k = report("high_band=%r" % args.high_band, args.files, runs["band"])
            print(f"  {args.high_band} / drop = {k / d:.3f}")
            band(args, paths)
        sos_amd.set_precision("bf16")
        return
    if args.link_channels:
        det = dnet.get_network()
        det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
        jm = jnet.get_network(MyConfig())
        jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
        det, jm = det.cuda().eval(), jm.cuda().eval()
        sos_amd.set_precision("mixed")
        with tempfile.TemporaryDirectory() as tmp:
            paths, secs = make_files(tmp, args.files, args.seed)
            forms = dict(unlinked=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "unlinked"), max_batch=args.max_batch),
                         linked=lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "linked"), max_batch=args.max_batch,
                                                                      link_channels=args.link_channels))
            for fn in forms.values():                                                     # warm-up of both forms
                fn()
            runs = {k: [] for k in forms}
            for _ in range(args.repeats):                                                 # the forms alternate
                for k, fn in forms.items():
                    runs[k].append(once(fn))
            print(f"{args.files} stereo s16 files at {RATE} Hz, {secs:.0f} s of audio x 2 channels, 'mixed' precision, {args.repeats} "
                  "alternating repeats (median, min, max)")
            u = report("link_channels=None", args.files, runs["unlinked"])
            k = report("link_channels=%r" % args.link_channels, args.files, runs["linked"])
            print(f"  linked / unlinked = {k / u:.3f}")
            link_launch(args, paths)
        sos_amd.set_precision("bf16")
        return
    if not args.skip_loop:
        det = dnet.get_network()
        det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
        jm = jnet.get_network(MyConfig())
        jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
        det, jm = det.cuda().eval(), jm.cuda().eval()
        sos_amd.set_precision("mixed")
        with tempfile.TemporaryDirectory() as tmp:
            paths, secs = make_files(tmp, args.files, args.seed)
            group = lambda: recordings.denoise_recordings(det, jm, paths, os.path.join(tmp, "group"), max_batch=args.max_batch)   # noqa: E731
            loop = lambda: per_file_loop(det, jm, paths, os.path.join(tmp, "loop"))                                            # noqa: E731
            ys, _, _ = audio_io.load_channels_batch_device(paths, sr=pipeline.SR)
            clips = [y[c] for y in ys for c in range(y.shape[0])]
            long_only = lambda: windows.denoise_long(det, jm, clips, max_batch=args.max_batch)                                 # noqa: E731
            group(), loop(), long_only()                                                  # warm-up of all forms
            runs = dict(group=[], loop=[], long_only=[])
            for _ in range(args.repeats):                                                 # the forms alternate
                runs["group"].append(once(group))
                runs["loop"].append(once(loop))
                runs["long_only"].append(once(long_only))
            print(f"{args.files} stereo s16 files at {RATE} Hz, {secs:.0f} s of audio x 2 channels, 'mixed' precision, {args.repeats} "
                  "alternating repeats (median, min, max)")
            g = report("denoise_recordings", args.files, runs["group"])
            lp = report("per file and channel", args.files, runs["loop"])
            d = report("denoise_long alone", args.files, runs["long_only"])
            print(f"  per file and channel / group = {lp / g:.2f}; share of the group call that is not denoise_long: {100 * (1 - d / g):.1f} %")
        sos_amd.set_precision("bf16")
    for amplitude in args.amplitudes:                            # decode is timed once, with the first amplitude below 1
        kernels(args, amplitude)


if __name__ == "__main__":
    main()
