"""resampling.py for audio that is still arriving: StreamResampler and StreamBandMerger, sessions of concurrent streams (session.py)
whose output is resample_device's and resample_merge_batch_device's bit for bit, with the state on the device
(csrc/stream_resample.hip, csrc/stream_band.hip)."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ragged
from . import session
from . import tools
from . import transform
from .resampling import KAISER_BEST, filter_on


class StreamResampler:
    """resample_device for audio that is still arriving: a session of `slots` concurrent streams at one pair of rates (a capture
    device, a call leg, a monitor feed at 48 / 44.1 / 16 / 8 kHz in front of the 14 kHz networks, and back).
      push({slot: chunk}) -> {slot: 1-D f32 GPU tensor}: chunks are 1-D float32 GPU tensors or numpy arrays of ANY length, 0
          included; a slot without an open stream begins one at output 0.  Returned are the outputs that have become final,
          possibly none, as views of one output buffer.
      close(slots) -> {slot: the rest}; the slots are free afterwards.      drop(slots): forgets streams without output.
    The concatenated output of a stream is BIT FOR BIT resample_device(the whole signal, orig_sr, target_sr, res_type, fix),
    whatever the chunking, the slot and the other streams: no truncated filter wings at the chunk edges, one running time
    register per stream (the rule: csrc/stream_resample.hip; float64 restatement tests/stream_resample_reference.py).  Output t
    is final once the R samples of its right wing are in (R = nwin // index_step: 64 when upsampling, 202 from 44.1 kHz and 219
    from 48 kHz down to 14 kHz), so the added latency is R + 1 input samples, 4.6 ms at 48 -> 14 kHz and at 14 -> 48 kHz.
    State lives on the device and is never downloaded: one ring of max_chunk + 2 R - 1 samples per slot (2 R - 1: the most that
    later outputs still read once the final ones are out).  The host knows every count from the chunk sizes and
    sos_stream_resample_ready, so after the first call (filter table, code object) no call waits for the device.  A push costs
    two launches whatever the number of slots (sos_stream_push_f32, sos_stream_resample_f32); a chunk larger than the free ring
    goes in pieces of two launches each.  orig_sr == target_sr passes chunks through.
    ValueError before any launch: slots outside 1 .. 65535, an unknown slot (push), a slot without an open stream or named twice
    (close, drop), a chunk that is not 1-D float32, an unsupported res_type, a ratio too small for the filter table
    (index_step < 1), max_chunk < 1, close of a stream too short to resample (the slot is named and free again; the other
    named slots stay open)."""

    def __init__(self, slots, orig_sr, target_sr, res_type="kaiser_best", fix=True, max_chunk=16384, device=None):
        if not 1 <= int(slots) <= ragged.MAX_CLIPS:
            raise ValueError(f"StreamResampler: 1 .. {ragged.MAX_CLIPS} slots, got {slots}")
        if res_type != "kaiser_best":
            raise ValueError("StreamResampler: res_type %r is not supported (the reference uses librosa's default 'kaiser_best')" % (res_type,))
        if int(max_chunk) < 1:
            raise ValueError(f"StreamResampler: max_chunk is at least 1 sample, got {max_chunk}")
        self.orig_sr, self.target_sr, self.fix = orig_sr, target_sr, bool(fix)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.ratio = float(target_sr) / orig_sr
        self.n_recv, self.t_done, self.base = [None] * int(slots), [0] * int(slots), [0] * int(slots)   # n_recv None: no stream
        self.ring = None
        if orig_sr == target_sr:
            return
        nwin = KAISER_BEST["num_zeros"] * 2 ** KAISER_BEST["precision"] + 1
        index_step = int(min(1.0, self.ratio) * 2 ** KAISER_BEST["precision"])
        if index_step < 1:
            raise ValueError("StreamResampler: ratio %g (%s->%s) is too small for the filter's %d-point table"
                             % (self.ratio, orig_sr, target_sr, 2 ** KAISER_BEST["precision"]))
        self.R = nwin // index_step
        self.capacity = int(max_chunk) + 2 * self.R - 1
        self.win, self.num_table = filter_on(self.device, self.ratio, res_type)
        self.ring = torch.zeros((int(slots), self.capacity), dtype=torch.float32, device=self.device)

    def _ready(self, n_recv):
        t, b = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().sos_stream_resample_ready(self.ratio, self.win.numel(), self.num_table, n_recv, C.byref(t), C.byref(b)),
                "sos_stream_resample_ready")
        return t.value, b.value

    def out_length(self, slot):
        """The number of samples the stream of `slot` gives in all if it is closed now (0: too short to resample)."""
        n = self.n_recv[slot]
        if self.ring is None:
            return n
        n_res = int(n * self.ratio)
        return (int(np.ceil(n * self.ratio)) if self.fix else n_res) if n_res >= 1 else 0

    def push(self, chunks):
        session.check_chunks("StreamResampler.push", chunks, len(self.n_recv))
        slots = list(chunks)
        for s in slots:
            if self.n_recv[s] is None:
                self.n_recv[s], self.t_done[s], self.base[s] = 0, 0, 0
        flat, offs = tools.stream_flat([chunks[s] for s in slots], self.device)
        left = [int(chunks[s].shape[0]) for s in slots]
        if self.ring is None:                                   # the same rate: the chunks themselves, on the device
            for i, s in enumerate(slots):
                self.n_recv[s] += left[i]
            return dict(zip(slots, ragged.split(flat, left) if flat is not None else [session.empty(self.device)] * len(slots)))
        # every count is the host's: what each slot emits in this call, hence where its outputs lie in the one buffer
        counts = [self._ready(self.n_recv[s] + left[i])[0] - self.t_done[s] for i, s in enumerate(slots)]
        where = {s: w - self.t_done[s] for s, w in zip(slots, ragged.offsets(counts).tolist())}      # of the stream's output 0
        out = torch.empty(sum(counts), dtype=torch.float32, device=self.device)
        # a slot's ring has room for at least min(left, max_chunk)
        for fill in session.fill_rounds(slots, offs, left, lambda s: (self.capacity - (self.n_recv[s] - self.base[s]), self.n_recv[s])):
            rows = []
            for s, _, take, _ in fill:
                self.n_recv[s] += take
                t_new, base = self._ready(self.n_recv[s])
                if t_new > self.t_done[s]:
                    rows.append((s, self.t_done[s], t_new, self.n_recv[s], t_new, where[s] + self.t_done[s]))
                self.t_done[s], self.base[s] = t_new, base
            tools.stream_push(flat, fill, self.ring)
            if rows:
                tools.stream_resample(self.ring, rows, self.ratio, self.win, self.num_table, out=out)
        return dict(zip(slots, ragged.split(out, counts)))

    def close(self, slots):
        slots = session.open_slots("StreamResampler.close", slots, self.n_recv)
        short = [s for s in slots if self.out_length(s) < 1 and self.ring is not None]
        if short:                                               # the other named streams stay open
            told = "; ".join("slot %d: Input signal length=%d is too small to resample from %s->%s"
                             % (s, self.n_recv[s], self.orig_sr, self.target_sr) for s in short)
            for s in short:
                self.n_recv[s] = None
            raise ValueError(f"StreamResampler.close: {told}")
        if self.ring is None:
            out, counts = None, [0] * len(slots)
        else:
            counts = [self.out_length(s) - self.t_done[s] for s in slots]
            where = ragged.offsets(counts).tolist()
            out = torch.empty(sum(counts), dtype=torch.float32, device=self.device)
            rows = [(s, self.t_done[s], self.out_length(s), self.n_recv[s], int(self.n_recv[s] * self.ratio), where[i])
                    for i, s in enumerate(slots) if counts[i]]
            if rows:
                tools.stream_resample(self.ring, rows, self.ratio, self.win, self.num_table, out=out)
        for s in slots:
            self.n_recv[s] = None
        return dict(zip(slots, ragged.split(out, counts) if out is not None else [session.empty(self.device)] * len(slots)))

    def drop(self, slots):
        for s in session.open_slots("StreamResampler.drop", slots, self.n_recv):
            self.n_recv[s] = None


class StreamBandMerger:
    """resample_merge_batch_device for audio that is still arriving: puts back, into live streams at native_sr > low_sr, the band
    above low_sr / 2 that a chain at low_sr never saw.  A session of `slots` concurrent streams; per stream x = the native audio,
    a = x at low_sr (an input StreamResampler's output), b = the chain's output for a (a StreamDenoiser's), and U = the resampling
    back:  out[t] = fmaf(g[t], x[t] - U(a)[t], U(b)[t]),  g = 1 with gains=None ('keep'), or band_gains_batch_device's frame gains
    with smooth_frames = `gains`, interpolated between frame centres ('follow').
      push({slot: (x_chunk, a_chunk, b_chunk)}) -> {slot: the outputs that became final}: each chunk a 1-D float32 GPU tensor or
          numpy array of ANY length, 0 included; a slot without an open stream begins one.  Views of one buffer.
      close(slots) -> {slot: the rest}; the slots are free afterwards.      drop(slots): forgets streams without output.
    The concatenated output of a stream has exactly one sample per sample of x and is BIT FOR BIT resample_merge_batch_device([x],
    [a], [b], low_sr, native_sr, gains)[0] for the whole signals (with gains = band_gains_batch_device([a], [b], hop, smooth_frames)
    under 'follow'), whatever the chunking, the slot and the other streams (the rule: csrc/stream_band.hip, include/sos_hip.h;
    float64 restatement tests/stream_band_reference.py).  Output t is final once b reaches R + 1 = 65 samples past its time (as
    a StreamResampler back to native_sr waits), under 'follow' also (smooth_frames + 2) hops past it: the frames of r that s
    around t averages must be whole.
    max_lag, in samples at low_sr: how far b may trail what x gives, ceil(n_x low_sr / native_sr) - m_b, after a push (so b trails
    a by no more); the rings are sized for it.
    State lives on the device and is never downloaded: ONE (3 slots, capacity) f32 tensor holds the x, a and b rings of every
    slot, capacity = max_chunk + ceil(ratio (max_lag + LAT)) + 2 samples with LAT = 64 ('keep') or max(64, (smooth_frames + 2) hop)
    -- what x can have pending, the largest of the three -- so 12 capacity bytes per slot; under 'follow' a ring of
    max(2 K + 1, K + ceil(64 / hop) + 2) + (max_lag + max_chunk) // hop + 3 frames of r in f64 per slot besides.  The host knows
    every count from the chunk sizes and sos_stream_band_ready, so after the first call (filter table, code object) no call
    waits for the device.  A push costs two launches under 'keep' whatever the number of slots (one sos_stream_push_f32 for all
    three rings, one sos_stream_band_merge_f32) and three under 'follow' (sos_stream_band_ratio_f64 between them); chunks larger
    than the free rings go in pieces of as many launches each.
    ValueError before any launch: native_sr <= low_sr, an unsupported res_type, smooth_frames outside 0 .. 16, slots outside
    1 .. 21845, max_lag < 0, max_chunk or hop < 1, an unknown slot or (close, drop) one named twice or without a stream, chunks
    that are not three 1-D float32 arrays, b ahead of a, a ahead of what x gives (m_a > ceil(n_x low_sr / native_sr)), b more than
    max_lag behind what x gives; at close a stream whose a does not cover its x (int(m ratio) < n) or without any b (the slot is
    named and free again; the other named slots stay open)."""

    def __init__(self, slots, low_sr, native_sr, max_lag, gains=None, hop=transform.HOP_LENGTH, max_chunk=16384,
                 res_type="kaiser_best", device=None):
        who = "StreamBandMerger"
        if not native_sr > low_sr:
            raise ValueError("%s: native_sr (%s) must exceed low_sr (%s): there is no band to put back otherwise" % (who, native_sr, low_sr))
        if res_type != "kaiser_best":
            raise ValueError("%s: res_type %r is not supported (the reference uses librosa's default 'kaiser_best')" % (who, res_type))
        if gains is not None and (isinstance(gains, bool) or not isinstance(gains, int) or not 0 <= gains <= 16):
            raise ValueError("%s: gains is None ('keep') or smooth_frames within 0 .. 16 ('follow'), got %r" % (who, gains))
        if not 1 <= int(slots) <= ragged.MAX_CLIPS // 3:
            raise ValueError(f"{who}: 1 .. {ragged.MAX_CLIPS // 3} slots, got {slots}")
        if int(max_lag) < 0 or int(max_chunk) < 1 or int(hop) < 1:
            raise ValueError(f"{who}: max_lag is at least 0 (got {max_lag}), max_chunk and hop at least 1 (got {max_chunk}, {hop})")
        self.low_sr, self.native_sr, self.smooth, self.hop, self.max_lag = low_sr, native_sr, gains, int(hop), int(max_lag)
        self.slots = int(slots)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.ratio, self.down = float(native_sr) / low_sr, float(low_sr) / native_sr
        self.R = KAISER_BEST["num_zeros"]
        K = gains
        lat = self.R if K is None else max(self.R, (K + 2) * self.hop)
        self.capacity = int(max_chunk) + int(np.ceil(self.ratio * (self.max_lag + lat))) + 2
        self.frames = 0 if K is None else max(2 * K + 1, K + -(-self.R // self.hop) + 2) + (self.max_lag + int(max_chunk)) // self.hop + 3
        self.win, self.num_table = filter_on(self.device, self.ratio, res_type)
        self.ring = torch.zeros((3 * self.slots, self.capacity), dtype=torch.float32, device=self.device)
        self.rring = None if K is None else torch.zeros((self.slots, self.frames), dtype=torch.float64, device=self.device)
        # per slot: samples received of x, a, b (None: no stream), outputs done, first a / b sample and r frame retained, frames of r written
        self.count = [None] * self.slots
        self.t_done, self.first, self.first_r, self.r_hi = ([0] * self.slots for _ in range(4))

    def _ready(self, m_b, n_x, memo=None):
        """memo: the answers of this call so far -- streams in lock step, and a push that takes one round, ask the same again."""
        if memo is not None and (m_b, n_x) in memo:
            return memo[m_b, n_x]
        v = [C.c_int64(0) for _ in range(5)]
        L.check(L.lib().sos_stream_band_ready(self.ratio, self.win.numel(), self.num_table, self.hop,
                                              -1 if self.smooth is None else self.smooth, m_b, n_x, *[C.byref(q) for q in v]),
                "sos_stream_band_ready")
        got = v[0].value, v[2].value, v[4].value                 # T, the first a / b sample, the first r frame
        if memo is not None:
            memo[m_b, n_x] = got
        return got

    def _low_length(self, n_x):
        return int(np.ceil(n_x * self.down))                     # resample_device's output length for n_x native samples

    def push(self, chunks):
        who = "StreamBandMerger.push"
        for s, c in chunks.items():
            if not isinstance(c, (tuple, list)) or len(c) != 3:
                raise ValueError(f"{who}: slot {s!r}: three chunks (x, a, b)")
        for k in range(3):
            session.check_chunks(who, {s: c[k] for s, c in chunks.items()}, self.slots)
        slots = list(chunks)
        after = {}
        for s in slots:
            n_x, m_a, m_b = (v + int(c.shape[0]) for v, c in zip(self.count[s] or (0, 0, 0), chunks[s]))
            m_x = self._low_length(n_x)
            if m_b > m_a or m_a > m_x or m_x - m_b > self.max_lag:
                raise ValueError(f"{who}: slot {s}: after this push x has {n_x} samples ({m_x} at {self.low_sr} Hz), a {m_a}, b {m_b}: "
                                 f"b may not run ahead of a, a not ahead of what x gives, and b may trail that by at most "
                                 f"max_lag = {self.max_lag} samples")
            after[s] = (n_x, m_a, m_b)
        for s in slots:
            if self.count[s] is None:
                self.count[s], self.t_done[s], self.first[s], self.first_r[s], self.r_hi[s] = (0, 0, 0), 0, 0, 0, 0
        S, K, hop = self.slots, self.smooth, self.hop
        rows_of = [k * S + s for s in slots for k in range(3)]      # the ring rows, x before a before b of a slot
        flat, offs = tools.stream_flat([chunks[s][k] for s in slots for k in range(3)], self.device)
        left = [int(chunks[s][k].shape[0]) for s in slots for k in range(3)]
        # every count is the host's: what each slot emits in this call, hence where its outputs lie in the one buffer
        memo = {}
        counts = [self._ready(after[s][2], after[s][0], memo)[0] - self.t_done[s] for s in slots]
        where = {s: w - self.t_done[s] for s, w in zip(slots, ragged.offsets(counts).tolist())}      # of the stream's output 0
        out = torch.empty(sum(counts), dtype=torch.float32, device=self.device)
        index, snap = {row: i for i, row in enumerate(rows_of)}, list(left)

        def state(row):
            k, s = divmod(row, S)
            n_x, m_a, m_b = self.count[s]
            if k == 0:
                return self.capacity - (n_x - self.t_done[s]), n_x
            if k == 1:
                return self.capacity - (m_a - self.first[s]), m_a
            i_a = index[S + s]
            free = min(self.capacity - (m_b - self.first[s]), m_a + (snap[i_a] - left[i_a]) - m_b)      # never ahead of a
            if K is not None:                                   # nor more whole frames than the ring of frames has room for
                free = min(free, (self.first_r[s] + self.frames + 1) * hop - 1 - m_b)
            return max(free, 0), m_b

        for fill in session.fill_rounds(rows_of, offs, left, state):
            if not fill:
                raise RuntimeError(f"{who}: the rings are full although max_lag holds (an internal error)")
            snap[:] = left
            for row, _, take, _ in fill:
                k, s = divmod(row, S)
                c = list(self.count[s])
                c[k] += take
                self.count[s] = tuple(c)
            ratio_rows, merge_rows = [], []
            for s in dict.fromkeys(row % S for row, _, _, _ in fill):
                n_x, m_a, m_b = self.count[s]
                if K is not None and m_b // hop > self.r_hi[s]:
                    ratio_rows.append((s, self.r_hi[s], m_b // hop, m_a, m_b))
                    self.r_hi[s] = m_b // hop
                t_new, first, first_r = self._ready(m_b, n_x, memo)
                if t_new > self.t_done[s]:
                    merge_rows.append((s, self.t_done[s], t_new, n_x, m_a, m_b, t_new, -1, self.r_hi[s], where[s] + self.t_done[s]))
                self.t_done[s], self.first[s], self.first_r[s] = t_new, first, first_r
            tools.stream_push(flat, fill, self.ring)
            if ratio_rows:
                tools.stream_band_ratio(self.ring, self.rring, ratio_rows, hop)
            if merge_rows:
                tools.stream_band_merge(self.ring, self.rring, merge_rows, self.ratio, self.win, self.num_table, hop, K, out)
        return dict(zip(slots, ragged.split(out, counts)))

    def close(self, slots):
        who = "StreamBandMerger.close"
        slots = session.open_slots(who, slots, self.count)
        bad = [s for s in slots if self.count[s][0] < 1 or int(self.count[s][1] * self.ratio) < self.count[s][0] or self.count[s][2] < 1]
        if bad:                                                 # the other named streams stay open
            told = "; ".join("slot %d: %d samples at %s Hz are not covered by the %d at %s Hz (they give %d), or the chain returned "
                             "none of them (%d)" % (s, self.count[s][0], self.native_sr, self.count[s][1], self.low_sr,
                                                    int(self.count[s][1] * self.ratio), self.count[s][2]) for s in bad)
            for s in bad:
                self.count[s] = None
            raise ValueError(f"{who}: {told}")
        K, hop = self.smooth, self.hop
        counts = [self.count[s][0] - self.t_done[s] for s in slots]
        where = ragged.offsets(counts).tolist()
        out = torch.empty(sum(counts), dtype=torch.float32, device=self.device)
        ratio_rows, merge_rows = [], []
        for i, s in enumerate(slots):
            n, m, mp = self.count[s]
            J = -(-m // hop)
            if K is not None and J > self.r_hi[s] and counts[i]:
                ratio_rows.append((s, self.r_hi[s], J, m, mp))
            if counts[i]:
                merge_rows.append((s, self.t_done[s], n, n, m, mp, int(mp * self.ratio), J if K is not None else -1, J, where[i]))
        if ratio_rows:
            tools.stream_band_ratio(self.ring, self.rring, ratio_rows, hop)
        if merge_rows:
            tools.stream_band_merge(self.ring, self.rring, merge_rows, self.ratio, self.win, self.num_table, hop, K, out)
        for s in slots:
            self.count[s] = None
        return dict(zip(slots, ragged.split(out, counts)))

    def drop(self, slots):
        for s in session.open_slots("StreamBandMerger.drop", slots, self.count):
            self.count[s] = None
