"""Float64 restatement of the windowing of long recordings (sos_amd.pipeline.window_plan / denoise_long and
csrc/ragged_window.hip), written from the rules alone and independent of the package: test infrastructure like the oracle.

A recording of n samples has the output length n_out = hop * (n // hop).  With `core` and `context` rounded up to multiples
of the hop it is cut into K = max(1, n_out // core) windows.  Window k owns the core [k core, (k + 1) core) of the output, the
last one up to n_out, and reads the source samples [max(k core - context, 0), (k + 1) core + context), the last one up to n.
Around every inner core boundary b the two neighbours are cross-faded over [b - context, b + context) with the weight
w(p) = (p - (b - context) + 0.5) / (2 context) of the later window; everywhere else the owner's row is the output."""
from collections import namedtuple

import numpy as np

HOP = 158                       # transform.HOP_LENGTH of the package's 14 kHz front end
MIN_FRAMES = 65                 # fewest STFT frames (1 + n // hop) of a clip the networks accept

Window = namedtuple("Window", "recording start samples core_start core_end")


def round_up(v, hop=HOP):
    return -(-int(v) // hop) * hop


def plan(ns, core, context, hop=HOP, min_frames=MIN_FRAMES):
    """The windows of recordings of `ns` samples, in recording order: a list of Window (start, core_start and core_end count
    samples of the recording).  ValueError for arguments or recordings the rules refuse."""
    core, context = round_up(core, hop), round_up(context, hop)
    if core < 2 * context:
        raise ValueError("core < 2 context: more than two windows would overlap")
    if core + context < min_frames * hop:
        raise ValueError("a window shorter than the networks accept")
    wins = []
    for r, n in enumerate(ns):
        if 1 + n // hop < min_frames:
            raise ValueError(f"recording {r} is too short")
        n_out = hop * (n // hop)
        K = max(1, n_out // core)
        for k in range(K):
            start = max(k * core - context, 0)
            if k == K - 1:
                wins.append(Window(r, start, n - start, k * core, n_out))
            else:
                wins.append(Window(r, start, (k + 1) * core + context - start, k * core, (k + 1) * core))
    return wins


def weights(context):
    """The later window's weights over an overlap zone of 2 context samples, float64."""
    return (np.arange(2 * context, dtype=np.float64) + 0.5) / (2 * context)


def stitch(wins, rows, context):
    """One recording's windows `wins` (in order) and their result rows (row k holds the samples from wins[k].start on)
    -> (out float64 of the recording's output length, blended bool: True inside the overlap zones)."""
    n_out = wins[-1].core_end
    out = np.zeros(n_out, dtype=np.float64)
    blended = np.zeros(n_out, dtype=bool)
    for w, row in zip(wins, rows):
        out[w.core_start:w.core_end] = np.asarray(row, dtype=np.float64)[w.core_start - w.start:w.core_end - w.start]
    if context:
        wt = weights(context)
        for j in range(len(wins) - 1):
            b = wins[j].core_end
            a = np.asarray(rows[j], dtype=np.float64)[b - context - wins[j].start:b + context - wins[j].start]
            c = np.asarray(rows[j + 1], dtype=np.float64)[b - context - wins[j + 1].start:b + context - wins[j + 1].start]
            out[b - context:b + context] = (1.0 - wt) * a + wt * c
            blended[b - context:b + context] = True
    return out, blended


def stitch_bound(wins, rows, context):
    """Per output sample of one recording: 4 * 2^-24 * max(|a|, |b|) of the two blended values inside the overlap zones (one
    rounding each for w and 1 - w, two products and a sum, contracted to an FMA or not), 0 elsewhere."""
    bound = np.zeros(wins[-1].core_end, dtype=np.float64)
    for j in range(len(wins) - 1 if context else 0):
        b = wins[j].core_end
        a = np.abs(np.asarray(rows[j], dtype=np.float64)[b - context - wins[j].start:b + context - wins[j].start])
        c = np.abs(np.asarray(rows[j + 1], dtype=np.float64)[b - context - wins[j + 1].start:b + context - wins[j + 1].start])
        bound[b - context:b + context] = 4.0 * 2.0 ** -24 * np.maximum(a, c)
    return bound


def table(wins, ns, hop=HOP, out_lens=None):
    """The int64 rows the kernels take for windows `wins` of recordings of `ns` samples lying back to back: {recording, source
    offset, samples, output offset, core start, core end, window start, row, previous, next}.  out_lens: the recordings' output
    lengths (default hop * (n // hop))."""
    ns = np.asarray(ns, dtype=np.int64)
    outs = hop * (ns // hop) if out_lens is None else np.asarray(out_lens, dtype=np.int64)
    src, dst = np.cumsum(ns) - ns, np.cumsum(outs) - outs
    tab = np.zeros((len(wins), 10), dtype=np.int64)
    for i, w in enumerate(wins):
        prev = i - 1 if i and wins[i - 1].recording == w.recording else -1
        nxt = i + 1 if i + 1 < len(wins) and wins[i + 1].recording == w.recording else -1
        tab[i] = (w.recording, src[w.recording] + w.start, w.samples, dst[w.recording] + w.start, w.core_start, w.core_end,
                  w.start, i, prev, nxt)
    return tab
