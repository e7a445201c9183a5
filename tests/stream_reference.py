"""Float64 restatement of the streaming rule (sos_amd.pipeline.StreamPlan / StreamDenoiser and csrc/stream_window.hip), written
from the rule alone and independent of the package: test infrastructure like window_reference.py, whose plan and stitch of the
complete recording it must reproduce exactly.

A stream that has received n_in samples has run the windows 0 .. k - 1.  Window k runs, as an inner window, as soon as
n_in >= (k + 2) core and reads [max(k core - context, 0), (k + 1) core + context).  After it the samples
[k core - context, (k + 1) core - context) are final (from 0 for k = 0); the first 2 context of them are blended with the saved
overlap of window k - 1, the rest is a copy of the window's row, and the row's samples [(k + 1) core - context,
(k + 1) core + context) are saved for the next window.  When the stream ends with n samples, one window is left, K - 1 with
K = max(1, hop * (n // hop) // core): it reads up to n and emits up to hop * (n // hop).  Pending samples live in a ring of
`capacity` >= 2 core + context samples, sample p at p % capacity."""
from collections import namedtuple

import numpy as np

import window_reference as R

Run = namedtuple("Run", "out wins emitted staged")


class Plan:
    """The windows of one stream: feed(n) -> [(k, Window)] that became ready, close() -> (k, Window) of the last one."""

    def __init__(self, core, context, hop=R.HOP, min_frames=R.MIN_FRAMES):
        R.plan([], core, context, hop, min_frames)              # the argument rules
        self.core, self.context, self.hop, self.min_frames = R.round_up(core, hop), R.round_up(context, hop), hop, min_frames
        self.n_in = self.k = 0

    def base(self):
        """The first sample a later window still reads."""
        return max(self.k * self.core - self.context, 0)

    def feed(self, n):
        self.n_in += n
        wins = []
        while self.n_in >= (self.k + 2) * self.core:
            start = self.base()
            wins.append((self.k, R.Window(0, start, (self.k + 1) * self.core + self.context - start, self.k * self.core,
                                          (self.k + 1) * self.core)))
            self.k += 1
        return wins

    def close(self):
        n = self.n_in
        if 1 + n // self.hop < self.min_frames:
            raise ValueError("the stream is too short")
        n_out = self.hop * (n // self.hop)
        assert max(1, n_out // self.core) == self.k + 1
        start = self.base()
        return self.k, R.Window(0, start, n - start, self.k * self.core, n_out)


def emitted(k, win, last, context):
    """[lo, hi) of the stream: what is final after window k."""
    return (win.core_start - context if k else win.core_start), (win.core_end if last else win.core_end - context)


def simulate(x, chunks, core, context, capacity=None, rows=None, hop=R.HOP, min_frames=R.MIN_FRAMES):
    """The stream `x` (1-D) fed in `chunks` (sizes that sum to len(x)) through a ring of `capacity` samples.  rows[k]: the result
    row of window k (it holds the samples from the window's start on); default: the window's own samples as staged out of the
    ring, cut to a multiple of the hop.  -> Run(out float64, wins, emitted ranges, staged rows)."""
    plan = Plan(core, context, hop, min_frames)
    core, context = plan.core, plan.context
    cap = 2 * core + context if capacity is None else capacity
    assert cap >= 2 * core + context and sum(chunks) == len(x)
    ring, state = np.zeros(cap, dtype=np.float64), dict(tail=None)
    out, wins, ranges, staged = [], [], [], []

    def run(k, win, last):
        st = ring[(win.start + np.arange(win.samples)) % cap].copy()
        row = np.asarray(st[:hop * (win.samples // hop)] if rows is None else rows[k], dtype=np.float64)
        lo, hi = emitted(k, win, last, context)
        piece = row[lo - win.start:hi - win.start].copy()
        if k and context:
            wt = R.weights(context)
            piece[:2 * context] = (1.0 - wt) * state["tail"] + wt * piece[:2 * context]
        if not last:
            state["tail"] = row[win.core_end - context - win.start:win.core_end + context - win.start].copy()
        out.append(piece), wins.append(win), ranges.append((lo, hi)), staged.append(st)

    at = 0
    for c in chunks:
        while c:
            take = min(c, cap - (plan.n_in - plan.base()))      # a chunk larger than the free ring goes in pieces
            assert take > 0
            ring[(plan.n_in + np.arange(take)) % cap] = x[at:at + take]
            at, c = at + take, c - take
            for k, win in plan.feed(take):
                run(k, win, False)
    run(*plan.close(), True)
    return Run(np.concatenate(out), wins, ranges, staged)
