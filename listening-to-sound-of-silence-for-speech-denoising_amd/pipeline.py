"""On-device inference chain: STFT -> detector -> threshold -> bits->sample-mask -> noise-interval
STFT -> JointModel -> mask apply -> ISTFT, with no host round trip.

Restates M1/predict.py:38-233 (detector pass) + M2/predict.py:255-326,377-447 (denoiser pass);
the reference hands results over through JSON/WAV files on disk, here the hand-off is the
`bits` tensor in HBM."""
import os

import torch

from . import get_mode, get_precision, precision_scope
from . import ragged
from . import tools
from . import transform

SR = 14000
FPS = 30.0
SIGMOID_THRESHOLD = 0.5     # M1/predict.py:30
MIN_FRAMES = 65             # ((T + 1) // 2 + 1) // 2 > 16, the reflect padding of InpaintNet's dilation-16 block


def n_video_frames(n_samples, sr=SR, fps=FPS):
    return int(round(n_samples / sr * fps))


# ---- the detector of the 'mixed' mode in two passes (round 5).  The only thing the pipeline takes from the detector is the SIGN
# of every frame's logit (M1/predict.py:117-119: sigmoid(logit) >= 0.5), and a 16-bit pass gets the sign wrong only where the
# logit lies inside its own error band around 0.  So: (1) the whole batch through the detector in fp16 (1x the MACs); (2) a device
# kernel marks the clips with ANY frame at |logit| < TWO_PASS_BAND x max(1, max_t |logit|) -- three times the fp16 logit tolerance
# the parity tests assert (tests/test_gpu_nets.py: 3e-3 of max |logit|; observed 1.5-1.8e-3); (3) ONLY the marked clips run again
# in the parity precision (bf16x3, 3x the MACs) through the kernels' ragged per-clip geometry -- unmarked clips get width 0 in
# every device table, their tiles exit at once, nothing is read back by the host (hipGraph-capturable); (4) marked clips take the
# parity logits, the others keep the fp16 ones.  Frame decisions equal the parity detector's: by recomputation inside the band,
# and outside it because an fp16 logit further than three tolerances from 0 has the reference's sign.  SOS_MIXED_TWO_PASS=0: every
# clip through the parity-precision detector (rounds 3-4).  The audio-visual variant and plain modes are untouched.
TWO_PASS = os.environ.get("SOS_MIXED_TWO_PASS", "1") != "0"
TWO_PASS_BAND = 3 * 3e-3
# Round 6: the band is relative to max(1, max_t |logit|, max_t scale_t) with scale_t = |W2| a_t + |b2| -- the magnitude
# of the TERMS of the last layer's dot product (one more 100 -> 1 launch in the fp16 pass).  An fp16 pass's logit error is
# proportional to the size of what is summed, not to the sum: a clip whose logits all hover near 0 by cancellation got a band of
# 0.009 from its own max |logit| while its error is that of its neighbours with large logits.  scale_t >= |logit_t|, so every clip
# the round-5 rule marked is still marked.  SOS_MIXED_BAND_SCALE=0: the round-5 rule (A/B).
BAND_SCALE = os.environ.get("SOS_MIXED_BAND_SCALE", "1") != "0"
_fixed_rag = {}


def detect(detector, S_mixed, n_frames, rag=None, return_mark=False, between=None):
    """Detector logits (B, n_frames) for the pipeline: the two-pass scheme above under set_precision('mixed'), one plain call
    otherwise.  rag: engine.Ragged of a variable-length batch.  between: optional callable run between the two passes (the
    pipeline starts the denoiser's encoder_x there: the second pass -- a few clips, or none -- cannot fill the chip)."""
    from . import engine as E
    # `between` fires where the chip starts to idle: before the (first) pass's BiLSTM if the detector offers the hook
    # (detector.networks.AudioVisualNet.forward(before_lstm=)), else after the pass
    hook = {}
    if between is not None and EARLY_X and "before_lstm" in getattr(getattr(detector.forward, "__code__", None), "co_varnames", ()):
        hook = dict(before_lstm=between)
        between = None
    if get_mode() != "mixed" or not TWO_PASS or getattr(detector, "video_feat", 0):
        lo = detector(s=S_mixed, v_num_frames=n_frames, rag=rag, **hook)
        return (lo, None) if return_mark else lo
    scale = None
    with precision_scope("fp16"):
        if BAND_SCALE and "return_scale" in getattr(getattr(detector.forward, "__code__", None), "co_varnames", ()):
            lo16, scale = detector(s=S_mixed, v_num_frames=n_frames, rag=rag, return_scale=True, **hook)
        else:
            lo16 = detector(s=S_mixed, v_num_frames=n_frames, rag=rag, **hook)
    if between is not None:
        between()
    base = rag
    if base is None:                                  # fixed-length batch: every clip has the same geometry (cached tables)
        B, T = S_mixed.shape[0], S_mixed.shape[3]
        key = (B, T, n_frames, str(S_mixed.device))
        base = _fixed_rag.get(key)
        if base is None:
            base = _fixed_rag[key] = E.Ragged([T] * B, S_mixed.device, n_vframes=[n_frames] * B)
            base.level(0), base.tab(base.n_vframes)
    mrag, mark = E.mask_ragged(base, lo16, TWO_PASS_BAND, [base.widths(0), base.n_vframes], scale=scale)
    lo3 = detector(s=S_mixed, v_num_frames=n_frames, rag=mrag)
    lo = torch.where(mark[:, None] != 0, lo3, lo16)
    return (lo, mark) if return_mark else lo


OVERLAP_X = os.environ.get("SOS_MIXED_OVERLAP_X", "1") != "0"      # A/B: encoder_x of the denoiser under the detector's low-occupancy tail
EARLY_X = os.environ.get("SOS_EARLY_X", "1") != "0"                # A/B: ... from the detector's BiLSTM on (every mode), not only between the two passes


def _begin_x(denoiser, S_mixed, rag=None, mode=None):
    """Start the denoiser's encoder_x on its branch stream if the model offers it (denoiser.networks.JointModel.begin_x).
    mode: the EFFECTIVE precision of the pipeline call, captured by denoise() / _denoise_group_padded() at their entry
    (get_precision(): honours an enclosing precision_scope, reads 'mixed' as 'fp16') -- the hook fires inside the detector's
    own scope (bf16x3 for the one-pass parity detector of 'mixed'), and the denoiser(...) call that later consumes the handle runs
    in the caller's mode: both sides of the hand-off must agree."""
    if not OVERLAP_X or not hasattr(denoiser, "begin_x"):
        return None
    with precision_scope(mode if mode is not None else get_precision()):
        return denoiser.begin_x(S_mixed, rag)


def two_pass_stats(device=None, reset=False):
    """(clips re-run in the parity precision, clips seen) by detect() on `device` so far; synchronises."""
    from . import engine as E
    c = E.band_count(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    out = tuple(int(v) for v in c.tolist())
    if reset:
        c.zero_()
    return out


@torch.no_grad()
def denoise(detector, denoiser, mixed, sr=SR, fps=FPS, bits=None, return_all=False):
    """mixed f32 (B, N) on the GPU -> denoised f32 (B, hop*(T-1)).  `bits` (uint8 (B, n_frames),
    1 = non-silent) overrides the detector (M2/predict.py's `recovered_prediction` input)."""
    B, N = mixed.shape
    mode = get_precision()            # the denoiser's mode, taken OUTSIDE the detector's precision scope
    S_mixed = transform.stft_batch(mixed)
    logits = mark = None
    started = []
    if bits is None:
        logits, mark = detect(detector, S_mixed, n_video_frames(N, sr, fps), return_mark=True,
                              between=lambda: started.append(_begin_x(denoiser, S_mixed, mode=mode)))
        bits, _ = tools.threshold_bits(logits, SIGMOID_THRESHOLD)
    mask, noise_sig = tools.bits_to_mask_batch(bits, float(sr) / fps, N, mixed)
    S_noise = transform.stft_batch(noise_sig)
    n_pred, crm = denoiser(S_mixed, S_noise, **({"started": started[0]} if started and started[0] is not None else {}))
    S_out = transform.batch_fast_icRM_sigmoid(S_mixed, crm)
    out = transform.istft_batch(S_out)
    if return_all:
        # mark (two-pass detector of the 'mixed' mode only): int32 (B,), 1 = the clip's logits are the parity-precision pass's
        return dict(out=out, logits=logits, bits=bits, mask=mask, n_pred=n_pred, crm=crm, S_mixed=S_mixed,
                    S_noise=S_noise, S_out=S_out, mark=mark)
    return out


def _group_geometry(ns, device, sr, fps, nv=None):
    """Per-clip frame / video-frame counts of a ragged group and their device tables (engine.Ragged).  nv: the clips' own
    numbers of frame decisions where they are given (the `bits` override) instead of following from sr and fps."""
    from . import engine as E
    T = [1 + n // transform.HOP_LENGTH for n in ns]
    nv = [n_video_frames(n, sr, fps) for n in ns] if nv is None else [int(v) for v in nv]
    if min(T) < MIN_FRAMES:
        # the U-Net's dilation-16 block reflects 16 columns at a quarter of the resolution: nn.ReflectionPad2d raises for a
        # shorter input (M2/networks.py:105,181), and so does the single-clip path (sos_conv2d_fwd's descriptor check)
        raise ValueError(f"clips need at least {MIN_FRAMES} STFT frames ({MIN_FRAMES * transform.HOP_LENGTH} samples); got {min(ns)} samples")
    rag = E.Ragged(T, device, n_vframes=nv, n_samples=ns)
    rag.tab(ns), rag.tab(nv), rag.level(0)          # uploaded here, not inside a later stream capture
    return rag


def _denoise_group_padded(detector, denoiser, wave, rag, sr, fps):
    """The launch sequence of one ragged group on its padded waveform buffer (B, max samples); no host <-> device traffic
    (capturable in a hipGraph).  Returns the padded output (B, hop * (max T - 1)) and the detector's logits / bits."""
    ns, nv = rag.n_samples, rag.n_vframes
    t_ns, t_nv = rag.tab(ns), rag.tab(nv)
    mode = get_precision()            # the denoiser's mode, taken OUTSIDE the detector's precision scope
    S_mixed = transform.stft_batch(wave, clip_samples=t_ns)
    started = []
    logits = detect(detector, S_mixed, max(nv), rag=rag, between=lambda: started.append(_begin_x(denoiser, S_mixed, rag, mode)))
    bits, _ = tools.threshold_bits(logits, SIGMOID_THRESHOLD)
    mask, noise_sig = tools.bits_to_mask_batch(bits, float(sr) / fps, wave.shape[1], wave, clip_frames=t_nv, clip_samples=t_ns)
    S_noise = transform.stft_batch(noise_sig, clip_samples=t_ns)
    n_pred, crm = denoiser(S_mixed, S_noise, rag=rag, **({"started": started[0]} if started and started[0] is not None else {}))
    S_out = transform.batch_fast_icRM_sigmoid(S_mixed, crm)
    return transform.istft_batch(S_out, clip_frames=rag.level(0)), logits, bits


def _pad_group(clips):
    ns = [int(c.numel()) for c in clips]
    wave = torch.zeros((len(clips), max(ns)), dtype=torch.float32, device=clips[0].device)
    for b, c in enumerate(clips):
        wave[b, :ns[b]] = c
    return wave, ns


def _denoise_group(detector, denoiser, clips, sr, fps):
    """One launch sequence for clips of DIFFERENT lengths: buffers sized for the longest clip, every kernel takes the
    clips' own sample / frame / video-frame counts from device tables (engine.Ragged), so each clip is computed exactly
    as if it were run alone: reflect padding of the STFT at its own end, zero / reflect conv borders at its own last
    frame, its own stride-2 sizes and transposed-conv crops, BiLSTM reverse pass from its own last frame, overlap-add
    normalisation of its own frame count."""
    wave, ns = _pad_group(clips)
    rag = _group_geometry(ns, wave.device, sr, fps)
    out, logits, bits = _denoise_group_padded(detector, denoiser, wave, rag, sr, fps)
    return [out[b, :transform.HOP_LENGTH * (rag.T[b] - 1)] for b in range(len(clips))], dict(logits=logits, bits=bits, rag=rag)


def _ragged_groups(clips, max_batch, max_columns):
    """Clips sorted by length (longest first) and cut into groups of <= max_batch clips and <= max_columns
    (clips x frames of the group's longest) spectrogram columns: lists of indices into `clips`."""
    return _length_groups([int(c.numel()) for c in clips], max_batch, max_columns)


def _length_groups(ns, max_batch, max_columns):
    """_ragged_groups of clips (or of windows, denoise_long) given by their lengths `ns` in samples."""
    order = sorted(range(len(ns)), key=lambda i: -ns[i])
    groups, j = [], 0
    while j < len(order):
        t_long = 1 + ns[order[j]] // transform.HOP_LENGTH
        nb = max(1, min(max_batch, max_columns // t_long, len(order) - j))
        groups.append(order[j:j + nb])
        j += nb
    return groups


def stage_group(clips, bits=None, n_bits=None, ratios=None):
    """Clips of one group (1-D f32 GPU tensors) -> the padded buffer(s) of the launch sequence in ONE launch
    (tools.ragged_stage): (wave (B, longest), ns) without `bits`; with `bits` -- the clips' frame decisions back to back on the
    GPU, `n_bits` of them per clip, `ratios` samples per frame per clip -- ((wave, masked, mask), ns), mask back to back in clip
    order."""
    ns = [int(c.numel()) for c in clips]
    flat = torch.cat(clips) if len(clips) > 1 else clips[0].contiguous()
    return tools.ragged_stage(flat, ragged.clip_table(ns, n_bits), max(ns), bits, ratios), ns


def _denoise_group_staged(denoiser, wave, masked, rag, signals=False):
    """The denoiser's launch sequence of one ragged group whose noise intervals are already cut out (`masked`): what
    _denoise_group_padded runs after its detector.  Returns the padded output (B, hop * (max T - 1)); signals=True: the padded
    ISTFTs (4 B, hop * (max T - 1)) of the mixed, the noise-interval, the predicted-noise and the output spectrograms, B rows
    each in that order -- the four signals the hand-off writes (M2/predict.py:515-560)."""
    t_ns = rag.tab(rag.n_samples)
    S_mixed = transform.stft_batch(wave, clip_samples=t_ns)
    S_noise = transform.stft_batch(masked, clip_samples=t_ns)
    n_pred, crm = denoiser(S_mixed, S_noise, rag=rag)
    S_out = transform.batch_fast_icRM_sigmoid(S_mixed, crm)
    if not signals:
        return transform.istft_batch(S_out, clip_frames=rag.level(0))
    return transform.istft_batch(torch.cat([S_mixed, S_noise, n_pred, S_out], dim=0), clip_frames=rag.tab(rag.T * 4))


def _denoise_ragged_bits(denoiser, clips, bits, sr, fps, max_batch, max_columns, return_all):
    """denoise_ragged with the first model's decisions given (`bits`): no detector; every group is staged by
    sos_ragged_stage_f32 in one launch (padded clips, noise intervals, sample masks at each clip's own sr / fps)."""
    import numpy as np
    if len(bits) != len(clips):
        raise ValueError("bits must hold one array of frame decisions per clip")
    ratios = [float(sr) / float(f) for f in ragged.per_clip(fps, len(clips), "fps")]      # fps: a scalar or one per clip
    for b in bits:
        if b.ndim != 1 or (b.dtype != torch.uint8 if torch.is_tensor(b) else b.dtype != np.uint8):
            raise ValueError("bits must be 1-D uint8 arrays or GPU tensors (1 = non-silent)")
    outs, extra = [None] * len(clips), [None] * len(clips)
    hop = transform.HOP_LENGTH
    for part in _ragged_groups(clips, max_batch, max_columns):
        group = [clips[i].contiguous().float() for i in part]
        device = group[0].device
        nb = [int(bits[i].shape[0]) for i in part]
        rag = _group_geometry([int(c.numel()) for c in group], device, sr, FPS, nv=nb)      # refuses short clips before any launch
        if all(torch.is_tensor(bits[i]) for i in part):
            d_bits = torch.cat([bits[i].to(device) for i in part])
        else:                                                                                # host arrays: one upload per group
            d_bits = torch.from_numpy(np.concatenate([bits[i].cpu().numpy() if torch.is_tensor(bits[i]) else bits[i] for i in part])).to(device)
        (wave, masked, mask), ns = stage_group(group, d_bits, nb, [ratios[i] for i in part])
        y = _denoise_group_staged(denoiser, wave, masked, rag, signals=return_all)
        B = len(part)
        bit_views, mask_views = (ragged.split(d_bits, nb), ragged.split(mask, ns)) if return_all else (None, None)
        for k, i in enumerate(part):
            n_out = hop * (rag.T[k] - 1)
            outs[i] = y[(3 * B if return_all else 0) + k, :n_out]
            if return_all:
                extra[i] = dict(bits=bit_views[k], mask=mask_views[k], noisy_input=y[k, :n_out],
                                noise_intervals=y[B + k, :n_out], predicted_full_noise=y[2 * B + k, :n_out])
    return (outs, extra) if return_all else outs


@torch.no_grad()
def denoise_ragged(detector, denoiser, clips, sr=SR, fps=FPS, max_batch=256, max_columns=65536, return_all=False, bits=None):
    """Variable-length inference (BASELINE configs[3]): `clips` = list of 1-D f32 GPU tensors of ANY lengths.
    The reference denoises one file at a time at its own length (M2/predict.py:377-447: no padding, so reflect
    padding, frame count and video-frame count follow the clip).  Here clips of different lengths share launches:
    they are sorted by length (the BiLSTM kernel steps 16 clips in lockstep, so neighbours should be similar) and cut
    into groups of <= max_batch clips and <= max_columns (clips x frames of the longest) spectrogram columns -- the
    memory budget of a launch sequence, ~0.5 MB of live activations per column -- and every group runs as ONE batch
    with per-clip geometry (_denoise_group).  Outputs come back in input order, each hop*(T-1) samples long.
    `bits` (one 1-D uint8 array or GPU tensor per clip, 1 = non-silent) overrides the detector as in denoise() -- M2/predict.py's
    `recovered_prediction` input; `detector` may then be None -- and `fps` may be one value per clip (the files of a data set
    carry their own `framerate`).  Grouping, the MIN_FRAMES refusal and the output order are the same; return_all then yields
    per clip its `bits`, the sample `mask` and the ISTFTs `noisy_input`, `noise_intervals`, `predicted_full_noise` of the mixed,
    the noise-interval and the predicted-noise spectrograms (with the output: the four signals the hand-off writes)."""
    for c in clips:
        if c.dim() != 1:
            raise ValueError("denoise_ragged expects 1-D waveforms")
    if bits is None and not isinstance(fps, (int, float)):
        raise ValueError("one fps per clip needs the clips' frame decisions (bits=): the detector's groups share one rate")
    if bits is not None:
        return _denoise_ragged_bits(denoiser, clips, bits, sr, fps, max_batch, max_columns, return_all)
    outs, extra = [None] * len(clips), [None] * len(clips)
    for part in _ragged_groups(clips, max_batch, max_columns):
        ys, info = _denoise_group(detector, denoiser, [clips[i].contiguous().float() for i in part], sr, fps)
        for k, i in enumerate(part):
            outs[i] = ys[k]
            if return_all:
                extra[i] = dict(logits=info["logits"][k, :info["rag"].n_vframes[k]], bits=info["bits"][k, :info["rag"].n_vframes[k]])
    return (outs, extra) if return_all else outs


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
    import numpy as np
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
    import numpy as np
    return np.searchsorted(plan[:, 0], np.arange(n_recordings + 1))


def _stitch_frames(kept, plan, wf, frames, sr, rates, core, context):
    """The windows' logits (`kept`: one row per window, plan[:, 7] says which) -> (logits, bits) of the recordings back to back:
    one sos_window_frames_stitch_f32 launch and one thresholding launch."""
    import numpy as np
    first = _first_windows(plan, len(frames))
    recs = np.stack([ragged.offsets(frames), np.asarray(frames, dtype=np.int64), first[:-1], np.diff(first)], axis=1)
    logits = tools.window_frames_stitch(kept, plan, wf, recs, [float(sr) / float(f) for f in rates], core, context)
    return logits, tools.threshold_bits(logits, SIGMOID_THRESHOLD)[0]


def _recording_frames(n_frames, ns, sr, rates):
    if n_frames is None:
        return [n_video_frames(n, sr, f) for n, f in zip(ns, rates)]
    if len(n_frames) != len(ns) or min(int(F) for F in n_frames) < 0:
        raise ValueError("n_frames must hold one non-negative number of frame decisions per recording")
    return [int(F) for F in n_frames]


@torch.no_grad()
def detect_long(detector, clips, sr=SR, fps=FPS, window_seconds=30.0, context_seconds=2.0, max_batch=256, max_columns=65536,
                n_frames=None, return_all=False):
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
    -> [(logits f32 (F,), bits uint8 (F,)) per recording], views of one buffer each, in input order; return_all adds per
    recording dict(plan=its window_plan rows (row = the order the windows ran in), windows=[logits per window]).
    ValueError before any launch as denoise_long."""
    import numpy as np
    clips = list(clips)
    if not clips:
        return ([], []) if return_all else []
    core, context, ns, plan = _long_plan("detect_long", clips, sr, window_seconds, context_seconds)
    rates = ragged.per_clip(fps, len(clips), "fps")
    frames = _recording_frames(n_frames, ns, sr, rates)
    wf = _window_frames(plan, sr, rates, frames)
    flat, _ = ragged.concat(clips)
    device = flat.device
    ms, W = plan[:, 2].tolist(), len(plan)
    kept = torch.empty((W, max(wf)), dtype=torch.float32, device=device)
    done = 0
    for part in _length_groups(ms, min(max_batch, ragged.MAX_CLIPS), max_columns):
        m, nv = [ms[i] for i in part], [wf[i] for i in part]
        wave = tools.window_stage(flat, np.ascontiguousarray(plan[part]), max(m))
        rag = _group_geometry(m, device, sr, FPS, nv=nv)
        logits = detect(detector, transform.stft_batch(wave, clip_samples=rag.tab(rag.n_samples)), max(nv), rag=rag)
        kept[done:done + len(part), :logits.shape[1]] = logits
        plan[part, 7] = np.arange(done, done + len(part))
        done += len(part)
    logits, bits = _stitch_frames(kept, plan, wf, frames, sr, rates, core, context)
    pairs = list(zip(ragged.split(logits, frames), ragged.split(bits, frames)))
    if not return_all:
        return pairs
    first = _first_windows(plan, len(clips))
    return pairs, [dict(plan=plan[first[r]:first[r + 1]], windows=[kept[plan[w, 7], :wf[w]] for w in range(first[r], first[r + 1])])
                   for r in range(len(clips))]


def _long_signal_rows(denoiser, flat, plan, d_bits, rec_table, ratios, fps_w, sr, max_batch, max_columns):
    """The groups of denoise_long(bits=, signals=True) and of the windowed hand-off: the windows of `plan` out of the recordings
    back to back in `flat`, staged with the recordings' masks (one sos_window_stage_masked_f32 launch per group) and run
    through _denoise_group_staged(signals=True).  -> kept (4, windows, longest row): the four signals' rows, plane by plane;
    plan[:, 7] is set to the row each window ran in.  Nothing goes to the host."""
    import numpy as np
    hop = transform.HOP_LENGTH
    ms, W = plan[:, 2].tolist(), len(plan)
    kept = torch.empty((4, W, hop * (max(ms) // hop)), dtype=torch.float32, device=flat.device)
    done = 0
    for part in _length_groups(ms, min(max_batch, ragged.MAX_CLIPS), max_columns):
        m, B = [ms[i] for i in part], len(part)
        rag = _group_geometry(m, flat.device, sr, FPS, nv=[max(1, n_video_frames(ms[i], sr, fps_w[i])) for i in part])
        wave, masked = tools.window_stage_masked(flat, d_bits, rec_table, ratios, np.ascontiguousarray(plan[part]), max(m))
        y = _denoise_group_staged(denoiser, wave, masked, rag, signals=True)
        kept[:, done:done + B, :y.shape[1]] = y.reshape(4, B, y.shape[1])
        plan[part, 7] = np.arange(done, done + B)
        done += B
    return kept


def _stitch_signals(kept, plan, context, recs=None, out_total=None):
    """The rows of _long_signal_rows cross-faded in ONE sos_window_stitch_planes_f32 launch.  Without `recs`: (4, total), the
    recordings' outputs back to back in each plane; with recs = host rows {base, pitch} per recording: the flat buffer of
    out_total floats with plane q of recording r from base_r + q * pitch_r on (the hand-off's file-major download)."""
    rows = plan.copy()
    rows[:, 2] = transform.HOP_LENGTH * (plan[:, 2] // transform.HOP_LENGTH)            # what a window's row holds
    return tools.window_stitch_planes(kept, rows, context, recs=recs, out_total=out_total)


@torch.no_grad()
def denoise_long(detector, denoiser, clips, sr=SR, fps=FPS, window_seconds=30.0, context_seconds=2.0, max_batch=256,
                 max_columns=65536, bits=None, return_all=False, stitch_bits=False, signals=False):
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
    stitch_bits together with bits, signals without decisions for the whole recording (neither bits nor stitch_bits)."""
    import numpy as np
    clips = list(clips)
    if signals and bits is None and not stitch_bits:
        raise ValueError("signals=True needs one decision stream per recording: pass bits=, or stitch_bits=True")
    if stitch_bits and bits is not None:
        raise ValueError("stitch_bits=True takes the decisions from the detector: it cannot be combined with bits=")
    if bits is None and not stitch_bits and not isinstance(fps, (int, float)):
        raise ValueError("one fps per recording needs the recordings' frame decisions (bits=, or stitch_bits=True): the "
                         "detector's groups share one rate")
    if bits is not None and len(bits) != len(clips):
        raise ValueError("bits must hold one array of frame decisions per recording")
    if not clips:
        return ([], []) if return_all or signals else []
    if stitch_bits:                                             # detect_long refuses what _long_plan refuses, before any launch
        pairs = detect_long(detector, clips, sr, fps, window_seconds, context_seconds, max_batch, max_columns)
        res = denoise_long(None, denoiser, clips, sr, fps, window_seconds, context_seconds, max_batch, max_columns,
                           bits=[b for _, b in pairs], return_all=return_all, signals=signals)
        if return_all:
            for e, (lg, _) in zip(res[1], pairs):
                e["logits"] = lg
        return res
    core, context, ns, plan = _long_plan("denoise_long", clips, sr, window_seconds, context_seconds)
    hop = transform.HOP_LENGTH
    W = len(plan)
    flat, _ = ragged.concat(clips)
    device = flat.device
    ms = plan[:, 2].tolist()
    if bits is not None:
        rates = ragged.per_clip(fps, len(clips), "fps")                                  # fps: a scalar or one per recording
        for b in bits:
            if b.ndim != 1 or (b.dtype != torch.uint8 if torch.is_tensor(b) else b.dtype != np.uint8):
                raise ValueError("bits must be 1-D uint8 arrays or GPU tensors (1 = non-silent)")
        nb = [int(b.shape[0]) for b in bits]
        if all(torch.is_tensor(b) for b in bits):
            d_bits = torch.cat([b.to(device) for b in bits])
        else:                                                                            # host arrays: one upload
            d_bits = torch.from_numpy(np.concatenate([b.cpu().numpy() if torch.is_tensor(b) else b for b in bits])).to(device)
        rec_table, ratios = ragged.clip_table(ns, nb), [float(sr) / float(f) for f in rates]
        fps_w = rates[plan[:, 0]]
    elif return_all:
        frames = [n_video_frames(n, sr, fps) for n in ns]
        wf = _window_frames(plan, sr, [fps] * len(clips), frames)
        kept_logits = torch.empty((W, max(wf)), dtype=torch.float32, device=device)
    lens = [hop * (n // hop) for n in ns]
    if signals:
        kept = _long_signal_rows(denoiser, flat, plan, d_bits, rec_table, ratios, fps_w, sr, max_batch, max_columns)
        four = _stitch_signals(kept, plan, context)             # (4, total): mixed, noise intervals, predicted noise, output
        outs = ragged.split(four[3], lens)
        extra = [dict(noisy_input=a, noise_intervals=b, predicted_full_noise=c)
                 for a, b, c in zip(*(ragged.split(four[q], lens) for q in range(3)))]
        if not return_all:
            return outs, extra
    else:
        kept = torch.empty((W, hop * (max(ms) // hop)), dtype=torch.float32, device=device)
        seen, done = [None] * W, 0
        for part in _length_groups(ms, min(max_batch, ragged.MAX_CLIPS), max_columns):
            m = [ms[i] for i in part]
            sub = np.ascontiguousarray(plan[part])
            if bits is None:
                wave = tools.window_stage(flat, sub, max(m))
                rag = _group_geometry(m, device, sr, fps)
                y, logits, wbits = _denoise_group_padded(detector, denoiser, wave, rag, sr, fps)
                if return_all:
                    kept_logits[done:done + len(part), :logits.shape[1]] = logits
                    for k, i in enumerate(part):
                        seen[i] = dict(logits=logits[k, :rag.n_vframes[k]], bits=wbits[k, :rag.n_vframes[k]])
            else:
                rag = _group_geometry(m, device, sr, FPS, nv=[max(1, n_video_frames(ms[i], sr, fps_w[i])) for i in part])
                wave, masked = tools.window_stage_masked(flat, d_bits, rec_table, ratios, sub, max(m))
                y = _denoise_group_staged(denoiser, wave, masked, rag)
            kept[done:done + len(part), :y.shape[1]] = y
            plan[part, 7] = np.arange(done, done + len(part))
            done += len(part)
        rows = plan.copy()
        rows[:, 2] = hop * (plan[:, 2] // hop)                                           # what a window's row holds
        outs = ragged.split(tools.window_stitch(kept, rows, context), lens)
        extra = [dict() for _ in clips]
    if not return_all:
        return outs
    first = _first_windows(plan, len(clips))
    for r, e in enumerate(extra):
        e["plan"] = plan[first[r]:first[r + 1]]
    if bits is None:
        logits, sbits = _stitch_frames(kept_logits, plan, wf, frames, sr, [fps] * len(clips), core, context)
        for r, (e, lg, b) in enumerate(zip(extra, ragged.split(logits, frames), ragged.split(sbits, frames))):
            e["windows"], e["logits"], e["bits"] = seen[first[r]:first[r + 1]], lg, b
    else:
        for e, b, n, ratio in zip(extra, ragged.split(d_bits, nb), ns, ratios):
            e["bits"], e["mask"] = b, tools.bits_to_mask_batch(b[None], ratio, n)[0]     # the whole recording's, made only here
    return outs, extra


class PipelinedDenoiser:
    """Serving loop over CONSECUTIVE batches (M2/predict.py:405-447 denoises file after file): batch i and batch i + 1 alternate
    between two HIP streams, so that the latency-bound tail of batch i -- the denoiser's BiLSTM on 8 workgroups, the FC head, the mask
    apply, the ISTFT -- runs under the chip-filling head of batch i + 1 (STFT, the detector's convolutions).  Each call returns
    (output, event): the output is complete once `event` has been waited for (event.synchronize() on the host, or
    stream.wait_event(event) on a consumer stream); synchronize() drains both streams.  The batches themselves are computed exactly
    as by denoise() (same kernels, same order per batch: bit-identical outputs).
    Lifetimes: `out` is allocated from the worker stream's pool and handed to the caller's stream -- it is recorded on
    the stream that is current at the call (out.record_stream), so its block is not reused while that stream still reads it; a
    consumer on yet another stream must record it there itself.  The first batch builds the caches every later batch shares
    (packed weights, geometry tables, transform tables) on streams[0]: the second batch, the first on streams[1], waits for it."""

    def __init__(self, detector, denoiser, sr=SR, fps=FPS):
        self.detector, self.denoiser, self.sr, self.fps = detector, denoiser, sr, fps
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.k = 0
        self._first = None

    @torch.no_grad()
    def __call__(self, mixed):
        st = self.streams[self.k & 1]
        caller = torch.cuda.current_stream()
        st.wait_stream(caller)                                # the input exists
        if self.k == 1 and self._first is not None:
            st.wait_event(self._first)                        # cold start: batch 0 built the shared caches on the other stream
        with torch.cuda.stream(st):
            out = denoise(self.detector, self.denoiser, mixed, self.sr, self.fps)
            ev = torch.cuda.Event()
            ev.record(st)
        if self.k == 0:
            self._first = ev
        self.k += 1
        mixed.record_stream(st)
        out.record_stream(caller)
        return out, ev

    def synchronize(self):
        for st in self.streams:
            st.synchronize()


class GraphedDenoiser:
    """hipGraph-captured inference chain (BASELINE configs[3]): the whole `denoise` launch sequence (~190 kernels
    for one (batch, length)) is captured once per shape and replayed, so a request costs one graph launch instead
    of ~190 host-side launches -- what bounds small-batch / streaming latency.  Shapes are exact (the reference
    pads nothing: M2/predict.py:377-447), the `max_graphs` most recently used graphs are kept.  Capture happens
    after two eager warm-up runs on a side stream (conv autotuning, weight packing and table uploads must not
    happen inside a capture).  Weights are read at replay time from the buffers packed at capture time, so the
    cache key carries the precision mode and the parameters' version counters (new weights -> new capture)."""

    def __init__(self, detector, denoiser, sr=SR, fps=FPS, max_graphs=16):
        self.detector, self.denoiser, self.sr, self.fps, self.max_graphs = detector, denoiser, sr, fps, max_graphs
        self._graphs = {}

    def reset(self):
        self._graphs.clear()

    def _capture(self, mixed):
        static_in = mixed.clone()
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(2):
                denoise(self.detector, self.denoiser, static_in, self.sr, self.fps)
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = denoise(self.detector, self.denoiser, static_in, self.sr, self.fps)
        return [graph, static_in, static_out, 0]

    @torch.no_grad()
    def __call__(self, mixed, clone=True):
        if mixed.dim() != 2 or not mixed.is_cuda or mixed.dtype != torch.float32:
            raise ValueError("GraphedDenoiser expects a float32 (B, N) GPU tensor")
        # precision mode and weight versions are part of the key: a graph replays the buffers packed at capture time
        from . import get_mode as get_precision
        wv = tuple(t._version for m in (self.detector, self.denoiser) for t in list(m.parameters()) + list(m.buffers()))
        key = (tuple(mixed.shape), mixed.device.index, get_precision(), hash(wv))
        entry = self._graphs.get(key)
        if entry is None:
            if len(self._graphs) >= self.max_graphs:
                del self._graphs[min(self._graphs, key=lambda k: self._graphs[k][3])]
            entry = self._graphs[key] = self._capture(mixed.contiguous())
        self._tick = getattr(self, "_tick", 0) + 1
        entry[3] = self._tick
        entry[1].copy_(mixed)
        entry[0].replay()
        return entry[2].clone() if clone else entry[2]

    def _capture_mixed(self, wave, rag):
        static_in = wave.clone()
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(2):
                _denoise_group_padded(self.detector, self.denoiser, static_in, rag, self.sr, self.fps)
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = _denoise_group_padded(self.detector, self.denoiser, static_in, rag, self.sr, self.fps)[0]
        return [graph, static_in, static_out, 0, rag]

    @torch.no_grad()
    def denoise_mixed(self, clips, max_batch=256, max_columns=65536):
        """BASELINE configs[3] as stated -- variable-length clips, hipGraph-captured forward: the ragged launch sequence of
        every group (pipeline.denoise_ragged's grouping, per-clip geometry in the kernels) is captured once per LENGTH MIX
        and replayed for new audio of the same lengths (a serving loop with fixed chunk sizes, a benchmark's repeated
        batch).  The per-clip tables are uploaded before the capture and kept alive with the graph."""
        from . import get_mode as get_precision
        for c in clips:
            if c.dim() != 1 or not c.is_cuda or c.dtype != torch.float32:
                raise ValueError("denoise_mixed expects 1-D float32 GPU waveforms")
        wv = tuple(t._version for m in (self.detector, self.denoiser) for t in list(m.parameters()) + list(m.buffers()))
        outs = [None] * len(clips)
        for part in _ragged_groups(clips, max_batch, max_columns):
            wave, ns = _pad_group([clips[i] for i in part])
            key = ("mixed", tuple(ns), wave.device.index, get_precision(), hash(wv))
            entry = self._graphs.get(key)
            if entry is None:
                if len(self._graphs) >= self.max_graphs:
                    del self._graphs[min(self._graphs, key=lambda k: self._graphs[k][3])]
                entry = self._graphs[key] = self._capture_mixed(wave, _group_geometry(ns, wave.device, self.sr, self.fps))
            self._tick = getattr(self, "_tick", 0) + 1
            entry[3] = self._tick
            entry[1].copy_(wave)
            entry[0].replay()
            T = entry[4].T
            for k, i in enumerate(part):
                outs[i] = entry[2][k, :transform.HOP_LENGTH * (T[k] - 1)].clone()
        return outs

    def denoise_ragged(self, clips, max_batch=64):
        """Equal-length buckets of `clips`, each replayed from its graph (streams of fixed-size chunks: the shapes repeat,
        so the graphs are reused; pipeline.denoise_ragged is the path for arbitrary mixed lengths)."""
        order = {}
        for i, c in enumerate(clips):
            if c.dim() != 1:
                raise ValueError("denoise_ragged expects 1-D waveforms")
            order.setdefault(int(c.numel()), []).append(i)
        outs = [None] * len(clips)
        for n, idx in sorted(order.items()):
            for j in range(0, len(idx), max_batch):
                part = idx[j:j + max_batch]
                y = self(torch.stack([clips[i] for i in part]))
                for k, i in enumerate(part):
                    outs[i] = y[k]
        return outs


class StreamPlan:
    """window_plan for ONE stream whose length is not known yet (host only; float64 restatement: tests/stream_reference.py).
    core, context: samples, rounded and refused as window_plan rounds and refuses them.  A stream that has received n_in samples
    has handed out the windows 0 .. k - 1:
      window k is ready, as an inner window, as soon as n_in >= (k + 2) core -- only then is it certain that window_plan of the
      final length does not make k the last window, which extends to the end; it reads [max(k core - context, 0),
      (k + 1) core + context);
      at close() the length n is known and exactly one window is left, K - 1 with K = max(1, hop * (n // hop) // core), which
      reads up to n.
    feed(n) -> the rows of the windows that became ready, close() -> the last one, as int64 (windows, 10) in window_plan's
    columns with the recording 0 and every offset counted in the stream: feed + close yield window_plan([n])'s rows in order.
    After window k the samples emitted(row) are final: [k core - context, (k + 1) core - context), from 0 for k = 0 and up to
    hop * (n // hop) for the last window; these ranges tile the output.  Between two windows at most 2 core + context samples
    are pending (`pending`: received and not below `base`, the first sample a later window still reads)."""

    def __init__(self, core, context):
        window_plan([], core, context)                          # the refusals are its own
        self.core, self.context = _hops(core), _hops(context)
        self.n_in = self.k = 0

    @property
    def base(self):
        return max(self.k * self.core - self.context, 0)

    @property
    def pending(self):
        return self.n_in - self.base

    def feed(self, n):
        import numpy as np
        if n < 0:
            raise ValueError(f"StreamPlan.feed: {n} samples")
        self.n_in += int(n)
        rows = []
        while self.n_in >= (self.k + 2) * self.core:
            k, cs, ce = self.k, self.k * self.core, (self.k + 1) * self.core
            start = max(cs - self.context, 0)
            rows.append((0, start, ce + self.context - start, start, cs, ce, start, k, k - 1 if k else -1, k + 1))
            self.k += 1
        return np.asarray(rows, dtype=np.int64).reshape(-1, tools.WINDOW_COLS)

    def close(self):
        """The last window's row (1, 10); ValueError for a stream below MIN_FRAMES frames, as window_plan refuses it.  Either
        way the plan is that of a new stream afterwards."""
        n, k = self.n_in, self.k
        self.n_in = self.k = 0
        row = window_plan([n], self.core, self.context)[-1:]
        assert int(row[0, 7]) == k, (n, k, row)
        return row

    def emitted(self, row):
        """[lo, hi) of the stream: the samples that are final after the window `row`."""
        return (int(row[4]) - self.context if row[8] >= 0 else int(row[4])), (int(row[5]) - self.context if row[9] >= 0 else int(row[5]))


class StreamDenoiser:
    """denoise_long for audio that is still arriving: a session of `slots` concurrent streams (a monitor feed, call channels, a
    capture still being written).  push() takes chunks of ANY size for any of the slots and returns, per slot, the denoised
    samples that have become final; close() ends streams and returns what was left; drop() forgets streams.  The concatenated
    output of a stream is denoise_long's result for the same audio with the same window_seconds / context_seconds: the plan
    (StreamPlan: window_plan without knowing the length), the windows' rows and the cross-fade are bit for bit the same, and with
    max_batch = 1 so is every sample, since every window then runs alone through the same launch sequence on the same shape
    (tests/test_gpu_stream_denoiser.py); with several windows in a group it differs as denoise_long's own batches differ.
    State lives on the device and is never downloaded: a ring of 2 core + context samples per slot (what has arrived and
    belongs to no finished window yet) and the overlap of each slot's last window, which the next one is blended with.  The host
    knows every count from the chunk sizes, so after the first calls (plans, tables, workspaces) no call waits for the device.
    push(): ONE sos_stream_push_f32 launch copies all chunks into their rings (a chunk larger than the free ring goes in pieces,
    one launch per piece of all slots); then, while a window is ready, one step with at most one window per slot: the ready
    windows grouped by max_batch / max_columns like denoise_long's, and per group one sos_stream_stage_f32 launch, the launch
    sequence of denoise_long's default path (_denoise_group_padded: the window's own detector pass with its own frame count)
    and one sos_stream_stitch_f32 launch.  close() runs the last windows of all named slots as one ragged call (their lengths
    differ) the same way.
    Latency: window k runs once (k + 2) core samples are in, so a sample is returned at most 2 core + context samples after it
    arrived (plus the compute time of its window); the first sample of a stream waits for 2 core.
    graph=True: per (windows, samples) of a group the launch sequence is captured once, exactly as
    GraphedDenoiser._capture_mixed captures it (two eager runs on a side stream first, the tables uploaded before the
    capture), the stage writes straight into the graph's input and the stitch reads its output; stage, stitch and their table
    uploads stay outside the graph.  close() runs eagerly: the last windows' lengths do not repeat.  `captures` counts them.
    in_sr / out_sr (default None: the streams are at `sr` on both sides and nothing below applies): audio at the rate of its
    device.  With in_sr, pushed chunks are at in_sr and pass through an audio_io.StreamResampler(slots, in_sr, sr) first; with
    out_sr, what push and close return has passed through a second one, sr -> out_sr.  Both are exact: the networks see, bit for
    bit, resample_device(the whole input, in_sr, sr), and the caller gets resample_device(the whole denoised stream, sr, out_sr)
    -- a live stream and a file of the same audio give the same samples (tests/test_gpu_stream_resample.py).  close() drains in
    order: the input resampler, the last window, the output resampler; drop() forgets all three.  Each side adds R + 1 samples
    of latency at its input rate (R = 219 at 48 -> 14 kHz, 64 at 14 -> 48 kHz: 4.6 ms each) and two launches per call.
    Not here: one decision stream per recording (denoise_long's stitch_bits needs frames of the future), given decisions
    (`bits=`), the four hand-off signals (`signals=`), and a res_type other than kaiser_best.
    ValueError before any launch: window_plan's argument rules, slots outside 1 .. 65535, a slot outside the slots (push) or
    without an open stream (close, drop), a chunk that is not 1-D float32, a closed stream below MIN_FRAMES frames at `sr` (the
    slot is named and free again; the other named slots stay open), StreamResampler's refusals of in_sr / out_sr."""

    def __init__(self, detector, denoiser, slots, sr=SR, fps=FPS, window_seconds=2.0, context_seconds=0.5, max_batch=256,
                 max_columns=65536, graph=False, device=None, in_sr=None, out_sr=None):
        self.core, self.context = _hops(round(window_seconds * sr)), _hops(round(context_seconds * sr))
        StreamPlan(self.core, self.context)
        if not 1 <= int(slots) <= ragged.MAX_CLIPS:
            raise ValueError(f"StreamDenoiser: 1 .. {ragged.MAX_CLIPS} slots, got {slots}")
        from .audio_io import StreamResampler
        self.rs_in = None if in_sr is None else StreamResampler(slots, in_sr, sr, device=device)
        self.rs_out = None if out_sr is None else StreamResampler(slots, sr, out_sr, max_chunk=self.core, device=device)   # a step's output
        self.detector, self.denoiser, self.sr, self.fps = detector, denoiser, sr, fps
        self.max_batch, self.max_columns, self.graph = min(int(max_batch), ragged.MAX_CLIPS), int(max_columns), bool(graph)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.capacity = 2 * self.core + self.context
        self.ring = torch.zeros((int(slots), self.capacity), dtype=torch.float32, device=self.device)
        self.tail = torch.zeros((int(slots), 2, max(2 * self.context, 1)), dtype=torch.float32, device=self.device)
        self.plans, self.parity = [None] * int(slots), [0] * int(slots)
        self._graphs, self.captures = {}, 0

    def _open(self, slots, who):
        slots = [slots] if isinstance(slots, int) else list(slots)
        for s in slots:
            if not isinstance(s, int) or not 0 <= s < len(self.plans) or self.plans[s] is None:
                raise ValueError(f"StreamDenoiser.{who}: slot {s!r} has no open stream")
        if len(set(slots)) != len(slots):
            raise ValueError(f"StreamDenoiser.{who}: a slot is named twice")
        return slots

    def _flat(self, chunks):
        """The chunks back to back in one device buffer (host arrays go up in one copy) and where each starts."""
        return tools.stream_flat(chunks, self.device)

    @torch.no_grad()
    def push(self, chunks):
        """chunks: {slot: 1-D float32 GPU tensor or numpy array, of any length, empty included}; a slot without an open stream
        begins one.  -> {slot: 1-D f32 GPU tensor of the samples that became final, possibly empty}."""
        import numpy as np
        for s, c in chunks.items():
            if not isinstance(s, int) or not 0 <= s < len(self.plans):
                raise ValueError(f"StreamDenoiser.push: unknown slot {s!r} (0 .. {len(self.plans) - 1})")
            if not (torch.is_tensor(c) or isinstance(c, np.ndarray)) or c.ndim != 1 or c.dtype != (torch.float32 if torch.is_tensor(c) else np.float32):
                raise ValueError(f"StreamDenoiser.push: slot {s}: a chunk is a 1-D float32 GPU tensor or numpy array")
            if torch.is_tensor(c):
                tools.L.require_cuda(c)
        if self.rs_in is not None:                              # chunks at in_sr -> what of them is final at the model rate
            chunks = self.rs_in.push(chunks)
        outs = self._push(chunks)
        return outs if self.rs_out is None else self.rs_out.push(outs)

    def _push(self, chunks):
        """push() for checked chunks at the model rate."""
        slots = list(chunks)
        for s in slots:
            if self.plans[s] is None:
                self.plans[s], self.parity[s] = StreamPlan(self.core, self.context), 0
        flat, offs = self._flat([chunks[s] for s in slots])
        left = [int(chunks[s].shape[0]) for s in slots]
        outs = {s: [] for s in slots}
        while any(left):
            rows, ready = [], []
            for i, s in enumerate(slots):
                plan = self.plans[s]
                take = min(left[i], self.capacity - plan.pending)
                if take:
                    rows.append((s, offs[i], take, plan.n_in))
                    offs[i], left[i] = offs[i] + take, left[i] - take
                    ready.append([(s, row) for row in plan.feed(take)])
            tools.stream_push(flat, rows, self.ring)              # a window is pending or the ring has room: rows is not empty
            while any(ready):                                   # a step: at most one window per slot
                self._run([q.pop(0) for q in ready if q], outs, self.graph)
        empty = torch.empty(0, dtype=torch.float32, device=self.device)
        return {s: (torch.cat(o) if len(o) > 1 else o[0]) if o else empty for s, o in outs.items()}

    @torch.no_grad()
    def close(self, slots):
        """Ends the streams of `slots` (an iterable of slots, or one): -> {slot: the remaining final samples}; the slots are free."""
        slots = self._open(slots, "close")
        hop = transform.HOP_LENGTH
        if self.rs_in is not None or self.rs_out is not None:
            return self._close_resampled(slots)
        short = [s for s in slots if 1 + self.plans[s].n_in // hop < MIN_FRAMES]
        if short:                                               # the other named streams stay open
            told = "; ".join(f"slot {s} got {self.plans[s].n_in} samples" for s in short)
            for s in short:
                self.plans[s] = None
            raise ValueError(f"StreamDenoiser.close: streams need at least {MIN_FRAMES} STFT frames ({MIN_FRAMES * hop} samples): {told}")
        items = [(s, self.plans[s].close()[0]) for s in slots]
        outs = {s: [] for s in slots}
        self._run(items, outs, False)
        for s in slots:
            self.plans[s] = None
        return {s: o[0] for s, o in outs.items()}

    def _close_resampled(self, slots):
        """close() with in_sr / out_sr: the input resampler is drained first, then the last window, then the output resampler."""
        hop = transform.HOP_LENGTH
        # the stream's length at the model rate once its input resampler is closed
        total = {s: self.rs_in.out_length(s) if self.rs_in is not None else self.plans[s].n_in for s in slots}
        short = [s for s in slots if 1 + total[s] // hop < MIN_FRAMES]
        if short:                                               # the other named streams stay open
            told = "; ".join(f"slot {s} got {total[s]} samples" for s in short)
            self._forget(short)
            raise ValueError(f"StreamDenoiser.close: streams need at least {MIN_FRAMES} STFT frames ({MIN_FRAMES * hop} samples at "
                             f"{self.sr} Hz): {told}")
        parts = {s: [] for s in slots}
        if self.rs_in is not None:
            for s, y in self._push(self.rs_in.close(slots)).items():
                parts[s].append(y)
        self._run([(s, self.plans[s].close()[0]) for s in slots], parts, False)
        for s in slots:
            self.plans[s] = None
        outs = {s: torch.cat(o) if len(o) > 1 else o[0] for s, o in parts.items()}
        if self.rs_out is None:
            return outs
        head, rest = self.rs_out.push(outs), self.rs_out.close(slots)
        return {s: torch.cat([head[s], rest[s]]) for s in slots}

    def _forget(self, slots):
        for s in slots:
            self.plans[s] = None
            for rs in (self.rs_in, self.rs_out):
                if rs is not None and rs.n_recv[s] is not None:
                    rs.drop([s])

    def drop(self, slots):
        """Forgets the streams of `slots` without output; the slots are free."""
        self._forget(self._open(slots, "drop"))

    def _run(self, items, outs, graph):
        """One window (slot, row of StreamPlan) per slot: staged, denoised and stitched in groups; appends to outs[slot]."""
        hop = transform.HOP_LENGTH
        ms = [int(row[2]) for _, row in items]
        for part in _length_groups(ms, self.max_batch, self.max_columns):
            group, m = [items[i] for i in part], [ms[i] for i in part]
            stage = [(s, int(row[6]), int(row[2])) for s, row in group]
            if graph:
                y = self._replay(m, stage)
            else:
                wave = tools.stream_stage(self.ring, stage, max(m))
                y = _denoise_group_padded(self.detector, self.denoiser, wave, _group_geometry(m, self.device, self.sr, self.fps),
                                          self.sr, self.fps)[0]
            table = [(s, i, int(row[6]), hop * (int(row[2]) // hop), int(row[4]), int(row[5]),
                      (tools.STREAM_HAS_PREV if row[8] >= 0 else 0) | (tools.STREAM_HAS_NEXT if row[9] >= 0 else 0), self.parity[s])
                     for i, (s, row) in enumerate(group)]
            out, lens = tools.stream_stitch(y, table, self.context, self.tail)
            for i, (s, row) in enumerate(group):
                outs[s].append(out[i, :lens[i]])
                if row[9] >= 0:
                    self.parity[s] ^= 1

    def _replay(self, m, stage):
        """The group's launch sequence from its graph, captured at the first group of these (windows, samples)."""
        wv = tuple(t._version for net in (self.detector, self.denoiser) for t in list(net.parameters()) + list(net.buffers()))
        key = (tuple(m), self.device.index, get_mode(), hash(wv))
        entry = self._graphs.get(key)
        if entry is None:                                       # _capture_mixed clones the staged rows into the graph's input
            entry = self._graphs[key] = GraphedDenoiser(self.detector, self.denoiser, self.sr, self.fps)._capture_mixed(
                tools.stream_stage(self.ring, stage, max(m)), _group_geometry(m, self.device, self.sr, self.fps))
            self.captures += 1
        else:
            tools.stream_stage(self.ring, stage, max(m), out=entry[1])
        entry[0].replay()
        return entry[2]
