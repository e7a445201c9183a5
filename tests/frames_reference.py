"""Float64 restatement of the frame stitch of long recordings (sos_amd.pipeline.detect_long and window_frames_stitch_kernel of
csrc/ragged_window.hip), written from the rule alone and independent of the package: test infrastructure like the oracle and
tests/window_reference.py, whose plan it takes.

A recording of n samples has F frame decisions (given, or n_video_frames(n, sr, fps)) and rho = sr / fps samples per frame.
Its windows k = 0 .. K - 1 (window_reference.plan) start at s_k, own the cores [cs_k, ce_k) and carry F_k =
max(1, n_video_frames(samples_k, sr, fps)) logits L_k each -- a recording of ONE window carries its own F.  The windows' frame
grids do not line up with the recording's (at 14 kHz and 30 fps a frame is 466.67 samples; windows start on multiples of the
hop), so frame i of the recording is placed by its centre:
    p      = (i + 0.5) rho                                       one rounded float64 multiply (i + 0.5 is exact)
    k      = min(floor(p) // core, K - 1)                        the owner; frames past the last core belong to the last window
    j_q(i) = clamp(floor((i + 0.5) - s_q / rho), 0, F_q - 1)     the frame of window q that holds p: one rounded divide, one
                                                                 rounded subtract.  F_q is a ROUNDED count, so the index of a
                                                                 neighbour can land one past its last frame: hence the clamp
    out[i] = L_k[j_k(i)]                                         outside the zones, an exact copy
and with context > 0, in the zones around the inner core boundaries (core >= 2 context: never both),
    k > 0     and p <  cs_k + context:  w = (p - (cs_k - context)) / (2 context),  out = (1 - w) L_{k-1}[j_{k-1}(i)] + w L_k[j_k(i)]
    k < K - 1 and p >= ce_k - context:  w = (p - (ce_k - context)) / (2 context),  out = (1 - w) L_k[j_k(i)] + w L_{k+1}[j_{k+1}(i)]
w is computed in float64 (one rounded subtract of an exact integer, one rounded divide) and rounded ONCE to float32; the kernel
blends in float32, this file in float64 with that same float32 w.
The bound of a blended frame, derived like window_reference.stitch_bound: the kernel rounds 1 - w (at most 2^-25 absolute, times
|a|), each of the two products and their sum (2^-24 relative each at most, on terms no larger than max(|a|, |b|) since the
weights are in [0, 1] and add up to 1 before rounding; an FMA contraction drops one of them): less than 4 * 2^-24 max(|a|, |b|),
the figure window_reference.stitch_bound uses for the same blend.  w itself adds nothing: it is the same float32 on both sides.
0 outside the zones."""
from collections import namedtuple

import numpy as np

import window_reference as W

Stitched = namedtuple("Stitched", "out blended bound owner index other other_index weight clamped")


def n_video_frames(n_samples, sr, fps):
    """The number of frame decisions of a clip of n_samples: Python's round (half to even) of the float64 n / sr * fps."""
    return int(round(n_samples / sr * fps))


def window_frames(wins, sr, fps, F=None):
    """F_k of one recording's windows; a recording of one window carries the recording's own F where that is given."""
    if len(wins) == 1 and F is not None:
        return [int(F)]
    return [max(1, n_video_frames(w.samples, sr, fps)) for w in wins]


def frame_index(i, start, rho, frames):
    """j_q(i) for frames i (array) of a window that starts at sample `start` and has `frames` frames; also the unclamped value."""
    raw = np.floor((np.asarray(i, dtype=np.float64) + 0.5) - np.float64(start) / np.float64(rho))
    return np.clip(raw, 0, frames - 1).astype(np.int64), raw.astype(np.int64)


def weight(p, zone_start, context):
    """The later window's weight at sample position p (float64 array) of the zone [zone_start, zone_start + 2 context):
    float64, rounded once to float32, returned as float64."""
    return ((np.asarray(p, dtype=np.float64) - np.float64(zone_start)) / np.float64(2 * context)).astype(np.float32).astype(np.float64)


def stitch(wins, logits, sr, fps, core, context, F=None):
    """One recording's windows `wins` (window_reference.Window, in order), their logit rows (row k holds at least F_k values),
    core and context in samples as the plan rounded them -> Stitched: out (float64, F values), blended (bool), bound (float64),
    owner / index (the window and its frame each output frame is taken from), other / other_index (the blended neighbour, -1
    outside the zones), weight (of the later window, 0 outside), clamped (how many indices the clamp changed)."""
    n = wins[-1].start + wins[-1].samples
    F = n_video_frames(n, sr, fps) if F is None else int(F)
    K = len(wins)
    rho = np.float64(sr) / np.float64(fps)
    fk = window_frames(wins, sr, fps, F)
    rows = [np.asarray(r, dtype=np.float64) for r in logits]
    i = np.arange(F, dtype=np.int64)
    p = (i.astype(np.float64) + 0.5) * rho
    owner = np.minimum(np.floor(p).astype(np.int64) // int(core), K - 1)
    out, bound = np.zeros(F, np.float64), np.zeros(F, np.float64)
    index, other, other_index = np.zeros(F, np.int64), np.full(F, -1, np.int64), np.full(F, -1, np.int64)
    wt, blended, clamped = np.zeros(F, np.float64), np.zeros(F, bool), 0
    for k, w in enumerate(wins):
        mine = owner == k
        jk, raw = frame_index(i, w.start, rho, fk[k])
        clamped += int((jk[mine] != raw[mine]).sum())
        index[mine] = jk[mine]
        out[mine] = rows[k][jk[mine]]
        if not context:
            continue
        for side, zone in ((-1, mine & (p < w.core_start + context) if k > 0 else None),
                           (1, mine & (p >= w.core_end - context) if k < K - 1 else None)):
            if zone is None or not zone.any():
                continue
            q = k + side
            jq, rawq = frame_index(i, wins[q].start, rho, fk[q])
            clamped += int((jq[zone] != rawq[zone]).sum())
            wz = weight(p[zone], (w.core_start if side < 0 else w.core_end) - context, context)
            own, nb = rows[k][jk[zone]], rows[q][jq[zone]]
            out[zone] = (1.0 - wz) * nb + wz * own if side < 0 else (1.0 - wz) * own + wz * nb
            bound[zone] = 4.0 * 2.0 ** -24 * np.maximum(np.abs(own), np.abs(nb))
            blended[zone], other[zone], other_index[zone], wt[zone] = True, q, jq[zone], wz
    return Stitched(out, blended, bound, owner, index, other, other_index, wt, clamped)
