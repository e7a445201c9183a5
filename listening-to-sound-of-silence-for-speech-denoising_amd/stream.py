"""Audio that is still arriving through the windowed chain of windows.py: StreamPlan is window_plan for a stream whose length is
not known yet, StreamDenoiser a session of concurrent streams with its state on the device (csrc/stream_window.hip)."""
import numpy as np
import torch

from . import ragged
from . import session
from . import tools
from . import transform
from .stream_resampling import StreamBandMerger, StreamResampler
from .pipeline import FPS, MIN_FRAMES, SR, _GraphCache, _length_groups, _padded_run
from .windows import _hops, _row_plan, window_plan


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
    GraphedDenoiser.denoise_mixed captures its groups (two eager runs on a side stream first, the tables uploaded before the
    capture), the stage writes straight into the graph's input and the stitch reads its output; stage, stitch and their table
    uploads stay outside the graph.  close() runs eagerly: the last windows' lengths do not repeat.  `captures` counts them.
    in_sr / out_sr (default None: the streams are at `sr` on both sides and nothing below applies): audio at the rate of its
    device.  With in_sr, pushed chunks are at in_sr and pass through an audio_io.StreamResampler(slots, in_sr, sr) first; with
    out_sr, what push and close return has passed through a second one, sr -> out_sr.  Both are exact: the networks see, bit for
    bit, resample_device(the whole input, in_sr, sr), and the caller gets resample_device(the whole denoised stream, sr, out_sr)
    -- a live stream and a file of the same audio give the same samples (tests/test_gpu_stream_resample.py).  close() drains in
    order: the input resampler, the last window, the output resampler; drop() forgets all three.  Each side adds R + 1 samples
    of latency at its input rate (R = 219 at 48 -> 14 kHz, 64 at 14 -> 48 kHz: 4.6 ms each) and two launches per call.
    high_band ('drop', the default: the path above, untouched): what comes back at out_sr > sr is band-limited to sr / 2 = 7 kHz,
    since the band above it never reaches the networks.  'keep' / 'follow' put it back as recordings.denoise_recordings(high_band=)
    does for files, with the same bits: they need in_sr == out_sr, and with in_sr > sr no output resampler is created -- an
    audio_io.StreamBandMerger takes its place (with in_sr <= sr there is no band, and the session is that of 'drop').  Per push
    the chunk at in_sr goes to the merger's x ring and through the input resampler, whose output goes to the merger's a ring
    and to the windows, whose output goes to the merger's b ring; the merger returns what is final: out[t] = fmaf(g[t], x[t] -
    U(a)[t], U(b)[t]), bit for bit resample_merge_batch_device of the whole signals ('follow': with band_gains_batch_device's
    gains at `smooth_frames`), exactly one sample per input sample (tests/test_gpu_stream_highband.py).  The merger's launches --
    one sos_stream_push_f32 for its three rings, under 'follow' one sos_stream_band_ratio_f64, one sos_stream_band_merge_f32 --
    replace the output resampler's two, and like stage and stitch they stay outside a captured graph.  Latency over 'drop': none
    under 'keep' (the output resampler waits for the same R + 1 = 65 samples at sr); under 'follow' an output also waits until
    (smooth_frames + 2) hops at sr lie past it, about 45 ms at smooth_frames = 2.  Memory: the merger's rings hold what the
    session can have pending, max_lag = 2 core + context plus the input resampler's wing at sr: 12 bytes per native sample of
    max_chunk + in_sr / sr (max_lag + 64, or (smooth_frames + 2) hop if that is more) per slot -- about 2.8 MB at 48 kHz with 2 s cores
    and 0.5 s context -- plus, under 'follow', 8 bytes per frame of r.  close() drains the input resampler, the last window, then
    the merger.
    Not here: one decision stream per recording (denoise_long's stitch_bits needs frames of the future), given decisions
    (`bits=`), the four hand-off signals (`signals=`), and a res_type other than kaiser_best.
    ValueError before any launch: window_plan's argument rules, slots outside 1 .. 65535, a slot outside the slots (push) or
    without an open stream (close, drop), a chunk that is not 1-D float32, a closed stream below MIN_FRAMES frames at `sr` (the
    slot is named and free again; the other named slots stay open), StreamResampler's refusals of in_sr / out_sr, an unknown
    high_band, one other than 'drop' with in_sr != out_sr, smooth_frames outside 0 .. 16."""

    def __init__(self, detector, denoiser, slots, sr=SR, fps=FPS, window_seconds=2.0, context_seconds=0.5, max_batch=256,
                 max_columns=65536, graph=False, device=None, in_sr=None, out_sr=None, high_band="drop", smooth_frames=2):
        self.core, self.context = _hops(round(window_seconds * sr)), _hops(round(context_seconds * sr))
        StreamPlan(self.core, self.context)
        if not 1 <= int(slots) <= ragged.MAX_CLIPS:
            raise ValueError(f"StreamDenoiser: 1 .. {ragged.MAX_CLIPS} slots, got {slots}")
        if high_band not in ("drop", "keep", "follow"):
            raise ValueError("StreamDenoiser: unknown high_band %r (one of drop, keep, follow)" % (high_band,))
        if high_band != "drop":
            if in_sr is None or in_sr != out_sr:
                raise ValueError("StreamDenoiser: high_band=%r needs in_sr == out_sr (got %r and %r): the band comes from the input"
                                 % (high_band, in_sr, out_sr))
            if isinstance(smooth_frames, bool) or not isinstance(smooth_frames, int) or not 0 <= smooth_frames <= 16:
                raise ValueError("StreamDenoiser: smooth_frames within 0 .. 16, got %r" % (smooth_frames,))
        band = high_band != "drop" and in_sr > sr
        self.rs_in = None if in_sr is None else StreamResampler(slots, in_sr, sr, device=device)
        self.rs_out = None if out_sr is None or band else StreamResampler(slots, sr, out_sr, max_chunk=self.core, device=device)   # a step's output
        self.merger = None
        if band:                                                # b trails a by the session's pending bound, a trails x by rs_in's wing
            lead = int(np.ceil((self.rs_in.R + 1) * sr / in_sr)) + 2
            self.merger = StreamBandMerger(slots, sr, in_sr, 2 * self.core + self.context + lead,
                                           gains=smooth_frames if high_band == "follow" else None, device=device)
        self.detector, self.denoiser, self.sr, self.fps = detector, denoiser, sr, fps
        self.max_batch, self.max_columns, self.graph = min(int(max_batch), ragged.MAX_CLIPS), int(max_columns), bool(graph)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.capacity = 2 * self.core + self.context
        self.ring = torch.zeros((int(slots), self.capacity), dtype=torch.float32, device=self.device)
        self.tail = torch.zeros((int(slots), 2, max(2 * self.context, 1)), dtype=torch.float32, device=self.device)
        self.plans, self.parity = [None] * int(slots), [0] * int(slots)
        self._graphs, self.captures = _GraphCache((detector, denoiser)), 0

    @torch.no_grad()
    def push(self, chunks):
        """chunks: {slot: 1-D float32 GPU tensor or numpy array, of any length, empty included}; a slot without an open stream
        begins one.  -> {slot: 1-D f32 GPU tensor of the samples that became final, possibly empty}."""
        session.check_chunks("StreamDenoiser.push", chunks, len(self.plans))
        if self.merger is not None:
            return self._push_band(chunks)
        if self.rs_in is not None:                              # chunks at in_sr -> what of them is final at the model rate
            chunks = self.rs_in.push(chunks)
        outs = self._push(chunks)
        return outs if self.rs_out is None else self.rs_out.push(outs)

    def _push_band(self, chunks):
        """push() with a band merger: x -> its ring and rs_in -> a -> its ring and the windows -> b -> its ring -> what is final."""
        slots = list(chunks)
        flat, _ = tools.stream_flat([chunks[s] for s in slots], self.device)      # host chunks go up once
        if flat is not None:
            chunks = dict(zip(slots, ragged.split(flat, [int(chunks[s].shape[0]) for s in slots])))
        a = self.rs_in.push(chunks)
        b = self._push(a)
        return self.merger.push({s: (chunks[s], a[s], b[s]) for s in slots})

    def _push(self, chunks):
        """push() for checked chunks at the model rate."""
        slots = list(chunks)
        for s in slots:
            if self.plans[s] is None:
                self.plans[s], self.parity[s] = StreamPlan(self.core, self.context), 0
        flat, offs = tools.stream_flat([chunks[s] for s in slots], self.device)
        left = [int(chunks[s].shape[0]) for s in slots]
        outs = {s: [] for s in slots}
        # a window is pending or the ring has room: a round's rows are not empty
        for rows in session.fill_rounds(slots, offs, left, lambda s: (self.capacity - self.plans[s].pending, self.plans[s].n_in)):
            ready = [[(s, row) for row in self.plans[s].feed(take)] for s, _, take, _ in rows]
            tools.stream_push(flat, rows, self.ring)
            while any(ready):                                   # a step: at most one window per slot
                self._run([q.pop(0) for q in ready if q], outs, self.graph)
        empty = session.empty(self.device)
        return {s: (torch.cat(o) if len(o) > 1 else o[0]) if o else empty for s, o in outs.items()}

    @torch.no_grad()
    def close(self, slots):
        """Ends the streams of `slots` (an iterable of slots, or one): -> {slot: the remaining final samples}; the slots are free."""
        slots = session.open_slots("StreamDenoiser.close", slots, self.plans)
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
            rest_in = self.rs_in.close(slots)
            for s, y in self._push(rest_in).items():
                parts[s].append(y)
        self._run([(s, self.plans[s].close()[0]) for s in slots], parts, False)
        for s in slots:
            self.plans[s] = None
        outs = {s: torch.cat(o) if len(o) > 1 else o[0] for s, o in parts.items()}
        if self.merger is not None:
            nothing = session.empty(self.device)
            head, rest = self.merger.push({s: (nothing, rest_in[s], outs[s]) for s in slots}), self.merger.close(slots)
            return {s: torch.cat([head[s], rest[s]]) for s in slots}
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
            if self.merger is not None and self.merger.count[s] is not None:
                self.merger.drop([s])

    def drop(self, slots):
        """Forgets the streams of `slots` without output; the slots are free."""
        self._forget(session.open_slots("StreamDenoiser.drop", slots, self.plans))

    def _run(self, items, outs, graph):
        """One window (slot, row of StreamPlan) per slot: staged, denoised and stitched in groups; appends to outs[slot]."""
        ms = [int(row[2]) for _, row in items]
        for part in _length_groups(ms, self.max_batch, self.max_columns):
            group, m = [items[i] for i in part], [ms[i] for i in part]
            stage = [(s, int(row[6]), int(row[2])) for s, row in group]
            if graph:
                y = self._replay(m, stage)
            else:
                wave = tools.stream_stage(self.ring, stage, max(m))
                y = self._group_run(m)(wave)
            held = _row_plan(np.stack([row for _, row in group]))[:, 2].tolist()
            table = [(s, i, int(row[6]), held[i], int(row[4]), int(row[5]),
                      (tools.STREAM_HAS_PREV if row[8] >= 0 else 0) | (tools.STREAM_HAS_NEXT if row[9] >= 0 else 0), self.parity[s])
                     for i, (s, row) in enumerate(group)]
            out, lens = tools.stream_stitch(y, table, self.context, self.tail)
            for i, (s, row) in enumerate(group):
                outs[s].append(out[i, :lens[i]])
                if row[9] >= 0:
                    self.parity[s] ^= 1

    def _group_run(self, m):
        return _padded_run(self.detector, self.denoiser, m, self.device, self.sr, self.fps)

    def _replay(self, m, stage):
        """The group's launch sequence from its graph, captured at the first group of these (windows, samples): the cache clones
        the staged rows into the graph's input, later groups are staged straight into it."""
        entry, captured = self._graphs.entry(tuple(m), self.device,
                                             lambda: (tools.stream_stage(self.ring, stage, max(m)), self._group_run(m)))
        self.captures += captured
        if not captured:
            tools.stream_stage(self.ring, stage, max(m), out=entry.input)
        entry.graph.replay()
        return entry.output
