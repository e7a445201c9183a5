"""Recordings of any length through the chain of pipeline.py in overlapping windows: the plan (window_plan), the one loop that
runs a plan's windows in length groups and keeps their rows (_run_windows), and what is built on it -- detect_long, denoise_long
in its three modes, and the windowed hand-off (handoff.py).  The blend itself is csrc/ragged_window.hip."""
import numpy as np
import torch

from . import ragged
from . import tools
from . import transform
from .pipeline import (FPS, MIN_FRAMES, SIGMOID_THRESHOLD, SR, _bits_on, _check_bits, _denoise_group_padded, _denoise_group_staged,
                       _group_geometry, _length_groups, detect, n_video_frames)


def _hops(samples):
    """`samples` rounded up to a multiple of the STFT hop."""
    hop = transform.HOP_LENGTH
    return -(-int(samples) // hop) * hop


def window_plan(ns, core, context):
    """Recordings of `ns` samples cut into overlapping windows (host only; float64 restatement: tests/window_reference.py).
    core, context: samples, rounded up to multiples of the hop; core >= 2 context (only neighbouring windows overlap) and
    core + context >= MIN_FRAMES hops (every window is a clip the networks accept).  A recording of n samples has the output
    length n_out = hop * (n // hop) and K = max(1, n_out // core) windows.  Window k owns the core [k core, (k + 1) core) of the
    output -- the last one up to n_out, so between core and 2 core samples; a recording shorter than 2 core is one window -- and
    reads the source samples [max(k core - context, 0), (k + 1) core + context), the last one up to n: it keeps the n % hop
    tail, so its reflect padding sees the real end.  Every window starts on a multiple of the hop and all but the last are
    multiples of the hop long, so a window's denoised row covers exactly [start, start + hop * (samples // hop)) of the output.
    -> host int64 (windows, 10), the rows of sos_window_stage_f32 / sos_window_stitch_f32 in recording order:
    {recording, source offset in the back-to-back buffer, samples, output offset of the window's start in the back-to-back
    outputs, core start, core end, window start, row of the window's result (its index here), previous window, next window
    (indices here, -1 at a recording's ends)}.
    ValueError: the argument rules above, or a recording with fewer than MIN_FRAMES STFT frames (named)."""
    hop = transform.HOP_LENGTH
    if core < 0 or context < 0:
        raise ValueError(f"window_plan: core and context are non-negative sample counts, got {core} and {context}")
    core, context = _hops(core), _hops(context)
    if core < 2 * context:
        raise ValueError(f"window_plan: core ({core} samples) must be at least twice the context ({context}): only neighbouring "
                         "windows may overlap")
    if core + context < MIN_FRAMES * hop:
        raise ValueError(f"window_plan: core + context ({core + context} samples) must be at least {MIN_FRAMES} hops "
                         f"({MIN_FRAMES * hop} samples)")
    ns = [int(n) for n in ns]
    src, dst = ragged.offsets(ns).tolist(), ragged.offsets([hop * (n // hop) for n in ns]).tolist()
    rows = []
    for r, n in enumerate(ns):
        if 1 + n // hop < MIN_FRAMES:
            raise ValueError(f"recording {r}: clips need at least {MIN_FRAMES} STFT frames ({MIN_FRAMES * hop} samples); got {n} samples")
        n_out = hop * (n // hop)
        K, first = max(1, n_out // core), len(rows)
        for k in range(K):
            last = k == K - 1
            cs, ce = k * core, n_out if last else (k + 1) * core
            start, end = max(cs - context, 0), n if last else ce + context
            rows.append((r, src[r] + start, end - start, dst[r] + start, cs, ce, start, first + k, first + k - 1 if k else -1,
                         -1 if last else first + k + 1))
    return np.asarray(rows, dtype=np.int64).reshape(-1, tools.WINDOW_COLS)


def _long_plan(who, clips, sr, window_seconds, context_seconds):
    """What detect_long and denoise_long share before their first launch: (core, context, ns, plan) of 1-D `clips`."""
    for c in clips:
        if c.dim() != 1:
            raise ValueError(f"{who} expects 1-D waveforms")
    core, context = _hops(round(window_seconds * sr)), _hops(round(context_seconds * sr))
    ns = [int(c.numel()) for c in clips]
    plan = window_plan(ns, core, context)
    if len(plan) > ragged.MAX_CLIPS:
        raise ValueError(f"{who}: {len(plan)} windows in one call (at most {ragged.MAX_CLIPS}): longer windows, or fewer recordings")
    return core, context, ns, plan


def _window_frames(plan, sr, rates, frames):
    """Frame decisions per window of a plan: F_k = max(1, n_video_frames(samples_k, sr, fps of its recording)); a recording of
    ONE window is that clip itself and carries the recording's own count (`frames`, one per recording)."""
    first = _first_windows(plan, len(frames))
    wf = [max(1, n_video_frames(int(m), sr, rates[int(r)])) for r, m in zip(plan[:, 0], plan[:, 2])]
    for r, F in enumerate(frames):
        if first[r + 1] - first[r] == 1:
            wf[first[r]] = max(1, int(F))
    return wf


def _first_windows(plan, n_recordings):
    """Index of each recording's first window in a plan (and the number of windows at the end)."""
    return np.searchsorted(plan[:, 0], np.arange(n_recordings + 1))


def _stitch_frames(kept, plan, wf, frames, sr, rates, core, context):
    """The windows' logits (`kept`: one row per window, plan[:, 7] says which) -> (logits, bits) of the recordings back to back:
    one sos_window_frames_stitch_f32 launch and one thresholding launch."""
    first = _first_windows(plan, len(frames))
    recs = np.stack([ragged.offsets(frames), np.asarray(frames, dtype=np.int64), first[:-1], np.diff(first)], axis=1)
    logits = tools.window_frames_stitch(kept, plan, wf, recs, [float(sr) / float(f) for f in rates], core, context)
    return logits, tools.threshold_bits(logits, SIGMOID_THRESHOLD)[0]


def _check_link(who, link, link_mode, n_recordings):
    """What can be refused of `link` / `link_mode` from the arguments alone."""
    if link_mode not in tools.LINK_MODES:
        raise ValueError(f"{who}: link_mode must be one of {sorted(tools.LINK_MODES)}, got {link_mode!r}")
    if link is not None and len(link) != n_recordings:
        raise ValueError(f"{who}: link must hold one group id (or None) per recording: {n_recordings}, got {len(link)}")


def _link_tables(link, ns, rates, frames):
    """tools.link_tables of `link`, host only.  ValueError: members of a group that differ in samples, fps or frames."""
    links, members, group = tools.link_tables(link, frames)
    for r, g in enumerate(group):
        m = int(members[links[g, 2]])                           # the group's first member
        if (ns[r], float(rates[r]), frames[r]) != (ns[m], float(rates[m]), frames[m]):
            raise ValueError(f"linked recordings share one frame grid: recording {r} has {ns[r]} samples, {float(rates[r])} fps and "
                             f"{frames[r]} frames, recording {m} of its group {link[r]!r} has {ns[m]}, {float(rates[m])} and {frames[m]}")
    return links, members, group


def _link_frames(kept, plan, wf, frames, sr, rates, core, context, tables, link_mode):
    """_stitch_frames for linked recordings (tables: _link_tables'): -> [(logits, bits) per recording], every member of a group
    the SAME two tensors, views of the groups' streams that ONE sos_window_frames_link_f32 launch makes for all groups."""
    links, members, group = tables
    first = _first_windows(plan, len(frames))
    recs = np.stack([ragged.offsets(frames), np.asarray(frames, dtype=np.int64), first[:-1], np.diff(first)], axis=1)
    logits, bits = tools.window_frames_link(kept, plan, wf, recs, [float(sr) / float(f) for f in rates], core, context, links,
                                            members, link_mode, SIGMOID_THRESHOLD)
    lg, b = ragged.split(logits, links[:, 1]), ragged.split(bits, links[:, 1])
    return [(lg[g], b[g]) for g in group]


def _recording_frames(n_frames, ns, sr, rates):
    if n_frames is None:
        return [n_video_frames(n, sr, f) for n, f in zip(ns, rates)]
    if len(n_frames) != len(ns) or min(int(F) for F in n_frames) < 0:
        raise ValueError("n_frames must hold one non-negative number of frame decisions per recording")
    return [int(F) for F in n_frames]


def _row_plan(plan):
    """The plan as the stitch kernels read it: samples = what a window's row holds, hop * (samples // hop)."""
    rows = plan.copy()
    rows[:, 2] = transform.HOP_LENGTH * (plan[:, 2] // transform.HOP_LENGTH)
    return rows


def _run_windows(plan, device, max_batch, max_columns, run_group, planes=None, width=None):
    """The windows of `plan` in length groups (_length_groups of their samples, at most ragged.MAX_CLIPS in one), every group's
    rows kept: -> kept f32 (windows, width), or (planes, windows, width), on `device`; width: default the longest row.
    run_group(part, sub_plan, m, rows) is the launch sequence of one group -- part: the windows' indices in the plan, sub_plan:
    their rows of it (contiguous), m: their samples, rows: the range of rows of `kept` they get -- and returns their rows
    (len(part), <= width), with `planes` (planes * len(part), <= width) plane by plane.  plan[:, 7], the row a window ran in, is
    written here and nowhere else: it is what every stitch kernel trusts.  Nothing goes to the host."""
    ms, W = plan[:, 2].tolist(), len(plan)
    width = int(_row_plan(plan)[:, 2].max()) if width is None else width
    kept = torch.empty((W, width) if planes is None else (planes, W, width), dtype=torch.float32, device=device)
    done = 0
    for part in _length_groups(ms, min(max_batch, ragged.MAX_CLIPS), max_columns):
        rows = range(done, done + len(part))
        y = run_group(part, np.ascontiguousarray(plan[part]), [ms[i] for i in part], rows)
        kept[..., done:rows.stop, :y.shape[1]] = y.reshape(kept.shape[:-2] + (len(part), y.shape[1]))
        plan[part, 7] = np.arange(done, rows.stop)
        done = rows.stop
    return kept


@torch.no_grad()
def detect_long(detector, clips, sr=SR, fps=FPS, window_seconds=30.0, context_seconds=2.0, max_batch=256, max_columns=65536,
                n_frames=None, return_all=False, link=None, link_mode="any"):
    """The detector half of denoise_long: ONE stream of frame decisions per recording of any length.  `clips` are cut, staged
    and grouped exactly as denoise_long does it (window_plan, one sos_window_stage_f32 launch, one STFT and one detect() call
    with per-window frame counts per group); every group's logits are kept in one (windows, most frames of a window) buffer,
    and after the last group ONE sos_window_frames_stitch_f32 launch places every frame of a recording by its centre -- the
    window whose core holds it gives the frame of its own grid that holds it, blended with the neighbour's within
    `context_seconds` of an inner core boundary (the rule: csrc/ragged_window.hip; float64: tests/frames_reference.py) -- and
    one tools.threshold_bits launch decides.  Nothing goes to the host between the groups.
    fps: a scalar or one value per recording.  n_frames: the recordings' numbers of decisions (a file's label is not always
    n_video_frames(samples, sr, fps) long); default n_video_frames.  A recording shorter than two cores is one window with
    exactly these frames: denoise_ragged's clip, logits and bits bit for bit.
    link: one group id per recording (None: a group of its own); recordings with equal ids -- the channels of a file -- share
    ONE decision stream.  The stitch and the threshold launch are then replaced by ONE sos_window_frames_link_f32 launch, which
    stitches every member, reduces the members' logits in recording order (link_mode 'any': the maximum, a frame is speech if
    any member has speech; 'mean': the f32 mean; numpy restatement tests/link_reference.py) and decides; every member of a
    group gets the SAME (logits, bits) tensors.  The members of a group must agree in samples, fps and frames.  link=None:
    nothing changes.
    -> [(logits f32 (F,), bits uint8 (F,)) per recording], views of one buffer each, in input order; return_all adds per
    recording dict(plan=its window_plan rows (row = the order the windows ran in), windows=[logits per window]).
    ValueError before any launch as denoise_long; also a `link` of the wrong length, an unknown link_mode, linked recordings
    that differ in samples, fps or frames."""
    clips = list(clips)
    _check_link("detect_long", link, link_mode, len(clips))
    if not clips:
        return ([], []) if return_all else []
    core, context, ns, plan = _long_plan("detect_long", clips, sr, window_seconds, context_seconds)
    rates = ragged.per_clip(fps, len(clips), "fps")
    frames = _recording_frames(n_frames, ns, sr, rates)
    wf = _window_frames(plan, sr, rates, frames)
    tables = None if link is None else _link_tables(link, ns, rates, frames)
    flat, _ = ragged.concat(clips)

    def run_group(part, sub, m, rows):
        nv = [wf[i] for i in part]
        wave = tools.window_stage(flat, sub, max(m))
        rag = _group_geometry(m, flat.device, sr, FPS, nv=nv)
        return detect(detector, transform.stft_batch(wave, clip_samples=rag.tab(rag.n_samples)), max(nv), rag=rag)

    kept = _run_windows(plan, flat.device, max_batch, max_columns, run_group, width=max(wf))
    if link is None:
        logits, bits = _stitch_frames(kept, plan, wf, frames, sr, rates, core, context)
        pairs = list(zip(ragged.split(logits, frames), ragged.split(bits, frames)))
    else:
        pairs = _link_frames(kept, plan, wf, frames, sr, rates, core, context, tables, link_mode)
    if not return_all:
        return pairs
    first = _first_windows(plan, len(clips))
    return pairs, [dict(plan=plan[first[r]:first[r + 1]], windows=[kept[plan[w, 7], :wf[w]] for w in range(first[r], first[r + 1])])
                   for r in range(len(clips))]


def _masked_group(denoiser, flat, d_bits, rec_table, ratios, fps_w, sr, signals):
    """_run_windows' run_group of given decisions (denoise_long(bits=), the windowed hand-off): the windows out of the recordings
    back to back in `flat`, staged with the recordings' masks in one sos_window_stage_masked_f32 launch, then
    _denoise_group_staged; signals=True: the four signals' rows (4 B, len), for planes=4."""
    def run_group(part, sub, m, rows):
        rag = _group_geometry(m, flat.device, sr, FPS, nv=[max(1, n_video_frames(n, sr, fps_w[i])) for i, n in zip(part, m)])
        wave, masked = tools.window_stage_masked(flat, d_bits, rec_table, ratios, sub, max(m))
        return _denoise_group_staged(denoiser, wave, masked, rag, signals=signals)
    return run_group


def _stitch_signals(kept, plan, context, recs=None, out_total=None):
    """The four signals' rows (4, windows, width) cross-faded in ONE sos_window_stitch_planes_f32 launch.  Without `recs`: (4, total), the
    recordings' outputs back to back in each plane; with recs = host rows {base, pitch} per recording: the flat buffer of
    out_total floats with plane q of recording r from base_r + q * pitch_r on (the hand-off's file-major download)."""
    return tools.window_stitch_planes(kept, _row_plan(plan), context, recs=recs, out_total=out_total)


@torch.no_grad()
def denoise_long(detector, denoiser, clips, sr=SR, fps=FPS, window_seconds=30.0, context_seconds=2.0, max_batch=256,
                 max_columns=65536, bits=None, return_all=False, stitch_bits=False, signals=False, link=None, link_mode="any"):
    """Recordings of ANY length, minutes and hours included: `clips` = list of 1-D f32 GPU waveforms, short and long mixed.
    denoise_ragged runs a recording as one clip, which ends at sos_conv2d_fwd's 4 GB image (about 16 minutes at 14 kHz), needs
    ~0.5 MB of activations per STFT column and steps both BiLSTMs serially through the whole file.  Here every recording is cut
    into overlapping windows (window_plan: cores of `window_seconds`, `context_seconds` more on each inner side; a recording
    shorter than two cores is one window, i.e. exactly denoise_ragged's clip), the windows of ALL recordings run as ordinary
    ragged clips -- sorted by length and grouped by max_batch / max_columns like denoise_ragged's clips, one
    sos_window_stage_f32 launch per group out of the one concatenated buffer -- and their outputs are cross-faded over the
    2 context samples around every core boundary (sos_window_stitch_f32).  Activation memory follows max_columns (a group of
    windows), not the file: a file below that budget runs as one group and saves nothing, so lower max_columns to save memory
    (EXPERIMENTS.md 3.14: a quarter of the default costs no time on a 10-minute file, one window per group does).
    Each window is a clip in its own right: its own reflect padding, detector pass, frame count n_video_frames(samples, sr,
    fps) and BiLSTM passes.  The context is what is paid so that a core does not see these artificial edges at full weight: the
    result APPROXIMATES the whole-file result and is not equal to it (EXPERIMENTS.md has the distance on random-weight networks).
    Windows of one recording fall into different groups, and a boundary needs both rows: every group's output rows are kept
    (one buffer of windows x longest window, 4 bytes per output sample and overlap) and stitched ONCE after the last group, in
    one launch.  Nothing goes to the host between the groups.
    `bits` (one 1-D uint8 array or GPU tensor per recording, 1 = non-silent; `fps` a scalar or one value per recording;
    `detector` may be None): the first model's decisions as in denoise_ragged.  Every group is staged by ONE
    sos_window_stage_masked_f32 launch, which evaluates the mask rule in the RECORDING's coordinates (its frames, its ratio, its
    last sample): a sample's mask does not depend on the window it lands in, the rows are bit for bit slices of
    tools.ragged_stage's full-length ones, and nothing of a recording's full length is allocated.
    stitch_bits=True: the decisions are the detector's, but ONE stream per recording -- detect_long first, then the `bits` path
    on its device-resident bits, bit for bit denoise_long(None, denoiser, clips, bits=<detect_long's bits>, fps=fps) -- where
    the default silences each window by that window's own detector pass, so that the two windows cross-faded around a core
    boundary may have been denoised with different noise intervals there.  `fps` may then be one value per recording.
    link / link_mode (with stitch_bits=True only): detect_long's -- recordings with equal group ids, the channels of a file, are
    silenced by ONE shared stream, so their noise floors drop in and out together: bit for bit denoise_long(None, denoiser,
    clips, bits=<the group's stream for each recording>, fps=fps).
    Outputs come back in input order, each hop * (n // hop) samples long, views into one buffer.  return_all adds per recording
    dict(plan=its window_plan rows (row = the order the windows ran in), windows=[dict(logits, bits) per window], logits, bits=
    the recording's stitched stream as detect_long makes it, one more small launch); with `bits` dict(plan, bits, mask=the
    sample mask at full length, made only here); with stitch_bits dict(plan, logits, bits, mask).
    signals=True (with `bits` or stitch_bits): the four signals the hand-off writes, not the output alone.  Every group runs
    _denoise_group_staged(signals=True), its (4 B, len) rows are kept in one (4, windows, longest) buffer, and after the last
    group ONE sos_window_stitch_planes_f32 launch cross-fades all four.  -> (outs, extra): outs as without `signals`, bit for
    bit; extra[r] holds `noisy_input`, `noise_intervals`, `predicted_full_noise` (the ISTFTs of the mixed, the noise-interval
    and the predicted-noise spectrograms, stitched), each as long as the output, plus return_all's keys if that is set.
    ValueError before any launch: window_plan's (a recording below MIN_FRAMES frames is named), more than 65535 windows,
    stitch_bits together with bits, signals without decisions for the whole recording (neither bits nor stitch_bits), link
    without stitch_bits, and what detect_long refuses of link and link_mode."""
    clips = list(clips)
    if link is not None and not stitch_bits:
        raise ValueError("link= shares the detector's one stream per recording between recordings: it needs stitch_bits=True (the "
                         "default mode decides per window, and bits= already is a decision)")
    _check_link("denoise_long", link, link_mode, len(clips))
    if signals and bits is None and not stitch_bits:
        raise ValueError("signals=True needs one decision stream per recording: pass bits=, or stitch_bits=True")
    if stitch_bits and bits is not None:
        raise ValueError("stitch_bits=True takes the decisions from the detector: it cannot be combined with bits=")
    if bits is None and not stitch_bits and not isinstance(fps, (int, float)):
        raise ValueError("one fps per recording needs the recordings' frame decisions (bits=, or stitch_bits=True): the "
                         "detector's groups share one rate")
    if bits is not None:
        _check_bits(bits, len(clips), "recording")
    if not clips:
        return ([], []) if return_all or signals else []
    if stitch_bits:                                             # detect_long refuses what _long_plan refuses, before any launch
        pairs = detect_long(detector, clips, sr, fps, window_seconds, context_seconds, max_batch, max_columns, link=link,
                            link_mode=link_mode)
        res = denoise_long(None, denoiser, clips, sr, fps, window_seconds, context_seconds, max_batch, max_columns,
                           bits=[b for _, b in pairs], return_all=return_all, signals=signals)
        if return_all:
            for e, (lg, _) in zip(res[1], pairs):
                e["logits"] = lg
        return res
    core, context, ns, plan = _long_plan("denoise_long", clips, sr, window_seconds, context_seconds)
    flat, _ = ragged.concat(clips)
    if bits is None:
        outs, extra = _long_detected(detector, denoiser, flat, plan, ns, core, context, sr, fps, max_batch, max_columns, return_all)
    else:
        outs, extra = (_long_signals if signals else _long_given)(denoiser, flat, plan, ns, context, bits, sr, fps, max_batch,
                                                                  max_columns, return_all)
    return (outs, extra) if return_all or signals else outs


def _out_lengths(ns):
    return [transform.HOP_LENGTH * (n // transform.HOP_LENGTH) for n in ns]


def _long_detected(detector, denoiser, flat, plan, ns, core, context, sr, fps, max_batch, max_columns, return_all):
    """denoise_long's default mode: every window silenced by its own detector pass (_denoise_group_padded), one
    sos_window_stitch_f32 launch.  -> (outs, extra or None)."""
    device = flat.device
    if return_all:
        frames = [n_video_frames(n, sr, fps) for n in ns]
        wf = _window_frames(plan, sr, [fps] * len(ns), frames)
        kept_logits = torch.empty((len(plan), max(wf)), dtype=torch.float32, device=device)
        seen = [None] * len(plan)

    def run_group(part, sub, m, rows):
        wave = tools.window_stage(flat, sub, max(m))
        rag = _group_geometry(m, device, sr, fps)
        y, logits, wbits = _denoise_group_padded(detector, denoiser, wave, rag, sr, fps)
        if return_all:
            kept_logits[rows.start:rows.stop, :logits.shape[1]] = logits
            for k, i in enumerate(part):
                seen[i] = dict(logits=logits[k, :rag.n_vframes[k]], bits=wbits[k, :rag.n_vframes[k]])
        return y

    kept = _run_windows(plan, device, max_batch, max_columns, run_group)
    outs = ragged.split(tools.window_stitch(kept, _row_plan(plan), context), _out_lengths(ns))
    if not return_all:
        return outs, None
    first = _first_windows(plan, len(ns))
    logits, sbits = _stitch_frames(kept_logits, plan, wf, frames, sr, [fps] * len(ns), core, context)
    return outs, [dict(plan=plan[first[r]:first[r + 1]], windows=seen[first[r]:first[r + 1]], logits=lg, bits=b)
                  for r, (lg, b) in enumerate(zip(ragged.split(logits, frames), ragged.split(sbits, frames)))]


def _given(bits, flat, plan, ns, sr, fps):
    """What the two modes with given decisions stage from: (the decisions back to back on the device, their counts, the
    recordings' table, their samples per frame, the frame rate of every window's recording)."""
    rates = ragged.per_clip(fps, len(ns), "fps")                                         # fps: a scalar or one per recording
    d_bits, nb = _bits_on(bits, flat.device)                                             # host arrays: one upload
    return d_bits, nb, ragged.clip_table(ns, nb), [float(sr) / float(f) for f in rates], rates[plan[:, 0]]


def _given_extra(extra, plan, d_bits, nb, ns, ratios):
    """return_all of the two modes with given decisions: per recording its plan rows, its bits and its sample mask."""
    first = _first_windows(plan, len(ns))
    for r, (e, b) in enumerate(zip(extra, ragged.split(d_bits, nb))):
        e["plan"], e["bits"] = plan[first[r]:first[r + 1]], b
        e["mask"] = tools.bits_to_mask_batch(b[None], ratios[r], ns[r])[0]               # the whole recording's, made only here
    return extra


def _long_given(denoiser, flat, plan, ns, context, bits, sr, fps, max_batch, max_columns, return_all):
    """denoise_long(bits=): the windows staged with the recordings' masks, one sos_window_stitch_f32 launch."""
    d_bits, nb, rec_table, ratios, fps_w = _given(bits, flat, plan, ns, sr, fps)
    kept = _run_windows(plan, flat.device, max_batch, max_columns,
                        _masked_group(denoiser, flat, d_bits, rec_table, ratios, fps_w, sr, signals=False))
    outs = ragged.split(tools.window_stitch(kept, _row_plan(plan), context), _out_lengths(ns))
    return outs, _given_extra([dict() for _ in ns], plan, d_bits, nb, ns, ratios) if return_all else None


def _long_signals(denoiser, flat, plan, ns, context, bits, sr, fps, max_batch, max_columns, return_all):
    """denoise_long(bits=, signals=True): the four signals' rows plane by plane, one sos_window_stitch_planes_f32 launch."""
    d_bits, nb, rec_table, ratios, fps_w = _given(bits, flat, plan, ns, sr, fps)
    kept = _run_windows(plan, flat.device, max_batch, max_columns,
                        _masked_group(denoiser, flat, d_bits, rec_table, ratios, fps_w, sr, signals=True), planes=4)
    four = _stitch_signals(kept, plan, context)                 # (4, total): mixed, noise intervals, predicted noise, output
    lens = _out_lengths(ns)
    extra = [dict(noisy_input=a, noise_intervals=b, predicted_full_noise=c)
             for a, b, c in zip(*(ragged.split(four[q], lens) for q in range(3)))]
    return ragged.split(four[3], lens), _given_extra(extra, plan, d_bits, nb, ns, ratios) if return_all else extra
