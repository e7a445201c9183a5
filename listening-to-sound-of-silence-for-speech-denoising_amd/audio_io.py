"""The wave front door: what the reference gets from `librosa.load(path, sr=14000)`
(M1/dataset.py:226, M2/predict.py:288,297,303) and hands to `librosa.output.write_wav(path, y, sr)`
(M2/predict.py:515-528), with the same names and argument meaning:

  load(path, sr=22050, mono=True, offset=0.0, duration=None, dtype=np.float32, res_type='kaiser_best') -> (y, sr)
  resample(y, orig_sr, target_sr, res_type='kaiser_best', fix=True, scale=False)
  load_batch(paths, ...) / resample_batch(ys, ...): the same for a list of files / signals of any lengths, in a number
      of launches and copies that does not grow with the list (`load_batch_device` / `resample_batch_device` stay in HBM)
  to_mono(y)
  write_wav(path, y, sr, norm=False)
and, beyond librosa's names, the channel-preserving pair under recordings.py (csrc/pcm_io.hip):
  load_channels_batch_device(paths, sr=None) / decode_planes_batch_device(arrs, kinds): every channel as an f32 plane
  encode_batch_device(planes, fmt, frames=None) + wave_container(...): planes -> s16 / s24 / s32 / u8 / f32 WAVE data, or
      G.711 'alaw' / 'ulaw' code bytes (telephone audio: WAVE tags 6 / 7, read by read_wave like the linear formats)
  g711_decode_device(codes, law) / g711_encode_device(x, law): the same two launches for one chunk of a live call leg
  band_gains_batch_device(lows_in, lows_out) / resample_merge_batch_device(natives, lows_in, lows_out, orig_sr, target_sr,
      gains=None): what a chain at a lower rate never saw of a signal, put back at its own rate (csrc/band_merge.hip)
  StreamResampler / StreamBandMerger: resample_device and resample_merge_batch_device for audio that is still arriving, with
      their bits, the state on the device (csrc/stream_resample.hip, csrc/stream_band.hip)

The RIFF container is parsed here on the host (bytes -> header fields + one frombuffer view, no per-sample
Python); sample conversion, channel mix-down and the band-limited resampler are HIP kernels
(csrc/wave_io.hip).  `load_device` keeps the result in HBM for the pipeline.  No CPU fallback."""
import ctypes as C
import os
import struct

import numpy as np
import torch

from . import _lib as L
from . import ragged
from . import session
from . import tools
from . import transform

# resampy 0.2.2 `kaiser_best`: 64 zero crossings, 2**9 table points per crossing, Kaiser beta, roll-off
KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)

_FMT = {"s16": 0, "s32": 1, "f32": 2, "u8": 3}
_filters = {}


class WaveFormatError(ValueError):
    pass


def sinc_window(num_zeros, precision, beta, rolloff):
    """Half of a Kaiser-windowed sinc low-pass, `2**precision` points per zero crossing (resampy
    filters.sinc_window with window=kaiser(beta)).  Returns (half_window f64, num_table)."""
    num_table = 2 ** precision
    n = num_table * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_table


def _filter_on(device, ratio, res_type):
    if res_type != "kaiser_best":
        raise ValueError("res_type %r is not supported (the reference uses librosa's default 'kaiser_best')" % (res_type,))
    key = (str(device), float(ratio))
    if key not in _filters:
        if "half" not in _filters:
            _filters["half"] = sinc_window(**KAISER_BEST)
        half, num_table = _filters["half"]
        w = half * ratio if ratio < 1 else half
        _filters[key] = (torch.from_numpy(w.astype(np.float32)).to(device), num_table)
    return _filters[key]


def resample_device(x, orig_sr, target_sr, res_type="kaiser_best", fix=True):
    """x f32 1-D on the GPU -> f32 1-D, ceil(n * ratio) samples (floor when fix=False)."""
    L.require_cuda(x)
    if x.dim() != 1 or x.dtype != torch.float32:
        raise ValueError("resample_device expects a 1-D float32 tensor")
    if orig_sr == target_sr:
        return x
    ratio = float(target_sr) / orig_sr
    n_in = x.numel()
    n_res = int(n_in * ratio)
    if n_res < 1:
        raise ValueError("Input signal length=%d is too small to resample from %s->%s" % (n_in, orig_sr, target_sr))
    n_out = int(np.ceil(n_in * ratio)) if fix else n_res
    win, num_table = _filter_on(x.device, ratio, res_type)
    x = x.contiguous()
    out = torch.empty(n_out, dtype=torch.float32, device=x.device)
    L.check(L.lib().sos_resample_f32(L.ptr(x), n_in, ratio, L.ptr(win), win.numel(), num_table, L.ptr(out), n_out,
                                     L.stream_ptr()), "sos_resample_f32")
    return out


def resample_batch_device(clips, orig_sr, target_sr, res_type="kaiser_best", fix=True):
    """resample_device of every clip of a list of 1-D f32 GPU tensors (any lengths) at one common ratio: a list of views
    into one output buffer, clip i with ceil(n_i * ratio) samples (int(n_i * ratio) with fix=False) that are bit for bit
    resample_device(clips[i]).  One torch.cat, one table upload and one launch (csrc/wave_io.hip) per 65535 clips."""
    clips = list(clips)
    L.require_cuda(*clips)
    for x in clips:
        if x.dim() != 1 or x.dtype != torch.float32:
            raise ValueError("resample_batch_device expects 1-D float32 tensors")
    if orig_sr == target_sr or not clips:
        return clips
    ratio = float(target_sr) / orig_sr
    win, num_table = _filter_on(clips[0].device, ratio, res_type)
    n_in = np.asarray([x.numel() for x in clips], dtype=np.int64)
    n_res = np.asarray([int(int(n) * ratio) for n in n_in], dtype=np.int64)
    for i, n in enumerate(n_res):
        if n < 1:
            raise ValueError("clip %d: Input signal length=%d is too small to resample from %s->%s"
                             % (i, n_in[i], orig_sr, target_sr))
    n_out = np.asarray([int(np.ceil(int(n) * ratio)) for n in n_in], dtype=np.int64) if fix else n_res
    n_valid = np.minimum(n_res, n_out)
    in_off, out_off = ragged.offsets(n_in), ragged.offsets(n_out)
    x = torch.cat(clips)
    out = torch.empty(int(n_out.sum()), dtype=torch.float32, device=x.device)
    h = L.lib()
    for c0 in range(0, len(clips), ragged.MAX_CLIPS):
        c1 = min(c0 + ragged.MAX_CLIPS, len(clips))
        i0, o0 = int(in_off[c0]), int(out_off[c0])
        tiles = -(-n_out[c0:c1] // L.RESAMPLE_CHUNK)
        tab = np.ascontiguousarray(np.stack([in_off[c0:c1] - i0, n_in[c0:c1], out_off[c0:c1] - o0, n_out[c0:c1], n_valid[c0:c1],
                                             ragged.offsets(tiles)]), dtype=np.int64)
        tab_dev = torch.from_numpy(tab).to(x.device)
        L.check(h.sos_resample_batch_f32(L.ptr(x[i0:]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0, ratio, L.ptr(win),
                                         win.numel(), num_table, L.ptr(out[o0:]), L.stream_ptr()), "sos_resample_batch_f32")
    return ragged.split(out, n_out)


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
        self.win, self.num_table = _filter_on(self.device, self.ratio, res_type)
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
        self.win, self.num_table = _filter_on(self.device, self.ratio, res_type)
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


def pcm_to_mono_device(pcm, fmt):
    """pcm: (n_frames, channels) device tensor of int16 / int32 / float32 / uint8, or of uint8 G.711 codes with fmt 'alaw' /
    'ulaw' -> mono f32 (n_frames,)."""
    L.require_cuda(pcm)
    pcm = pcm.contiguous()
    n, ch = pcm.shape
    out = torch.empty(n, dtype=torch.float32, device=pcm.device)
    if fmt in G711:
        L.check(L.lib().sos_g711_to_mono_f32(L.ptr(pcm), G711[fmt][0], ch, n, L.ptr(out), L.stream_ptr()), "sos_g711_to_mono_f32")
    else:
        L.check(L.lib().sos_pcm_to_mono_f32(L.ptr(pcm), _FMT[fmt], ch, n, L.ptr(out), L.stream_ptr()), "sos_pcm_to_mono_f32")
    return out


# ------------------------------------------------------------------------------------ RIFF/WAVE container
def read_wave(path):
    """Parse a RIFF/WAVE file -> (samples ndarray (n_frames, channels) in a kernel format, fmt, sample rate).
    PCM 8/16/24/32-bit, IEEE float 32/64, G.711 A-law / mu-law (tags 6 / 7 with 8 bits: the uint8 code bytes, fmt 'alaw' /
    'ulaw'), WAVE_FORMAT_EXTENSIBLE wrappers of those."""
    return read_wave_info(path)[:3]


def read_wave_info(path):
    """read_wave plus what the file itself stores: (samples, fmt, sample rate, info) with info = dict(tag, bits, channels, rate,
    frames) -- `bits` as stored, so 24 stays 24 although the samples are carried as s32, and 64 stays 64 although they are
    carried as f32."""
    with open(path, "rb") as fp:
        buf = bytearray(os.fstat(fp.fileno()).st_size)       # writable backing store: the sample view goes to torch
        fp.readinto(buf)
    if len(buf) < 12 or buf[:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise WaveFormatError("%s: not a RIFF/WAVE file" % path)
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(buf):
        cid, size = buf[pos:pos + 4], struct.unpack_from("<I", buf, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if size < 16:
                raise WaveFormatError("%s: short fmt chunk" % path)
            tag, ch, rate, _, align, bits = struct.unpack_from("<HHIIHH", buf, body)
            if tag == 0xFFFE and size >= 26:                 # WAVE_FORMAT_EXTENSIBLE: the sub-format GUID's first word
                tag = struct.unpack_from("<H", buf, body + 24)[0]
            fmt = (tag, ch, rate, align, bits)
        elif cid == b"data":
            data = memoryview(buf)[body:min(body + size, len(buf))]
            break
        pos = body + size + (size & 1)
    if fmt is None or data is None:
        raise WaveFormatError("%s: missing fmt or data chunk" % path)
    tag, ch, rate, align, bits = fmt
    if ch < 1:
        raise WaveFormatError("%s: no channels" % path)
    width = bits // 8
    n = len(data) // (width * ch)
    data = data[:n * width * ch]
    if tag == 1 and bits == 16:
        arr, kind = np.frombuffer(data, dtype="<i2"), "s16"
    elif tag == 1 and bits == 8:
        arr, kind = np.frombuffer(data, dtype=np.uint8), "u8"
    elif tag == 1 and bits == 32:
        arr, kind = np.frombuffer(data, dtype="<i4"), "s32"
    elif tag == 1 and bits == 24:                           # widen to the top three bytes of an int32
        b3 = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3)
        arr = np.zeros((b3.shape[0], 4), dtype=np.uint8)
        arr[:, 1:] = b3
        arr, kind = arr.view("<i4").reshape(-1), "s32"
    elif tag == 3 and bits == 32:
        arr, kind = np.frombuffer(data, dtype="<f4"), "f32"
    elif tag == 3 and bits == 64:
        arr, kind = np.frombuffer(data, dtype="<f8").astype(np.float32), "f32"
    elif (tag, bits) in _G711_KIND:                         # the code bytes as they are: the kernels expand them
        arr, kind = np.frombuffer(data, dtype=np.uint8), _G711_KIND[tag, bits]
    else:
        raise WaveFormatError("%s: unsupported WAVE format tag %d with %d bits" % (path, tag, bits))
    return arr.reshape(n, ch), kind, rate, dict(tag=tag, bits=bits, channels=ch, rate=rate, frames=n)


def wave_info(path):
    """read_wave_info's `info` from the chunk headers alone (the samples are not read), with the same refusals."""
    with open(path, "rb") as fp:
        size_all = os.fstat(fp.fileno()).st_size
        head = fp.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise WaveFormatError("%s: not a RIFF/WAVE file" % path)
        fmt, nbytes = None, None
        while True:
            ck = fp.read(8)
            if len(ck) < 8:
                break
            cid, size = ck[:4], struct.unpack("<I", ck[4:])[0]
            if cid == b"fmt ":
                body = fp.read(size + (size & 1))
                if size < 16 or len(body) < 16:
                    raise WaveFormatError("%s: short fmt chunk" % path)
                tag, ch, rate, _, _, bits = struct.unpack_from("<HHIIHH", body, 0)
                if tag == 0xFFFE and size >= 26 and len(body) >= 26:
                    tag = struct.unpack_from("<H", body, 24)[0]
                fmt = (tag, ch, rate, bits)
            elif cid == b"data":
                nbytes = max(0, min(size, size_all - fp.tell()))
                break
            else:
                fp.seek(size + (size & 1), os.SEEK_CUR)
    if fmt is None or nbytes is None:
        raise WaveFormatError("%s: missing fmt or data chunk" % path)
    tag, ch, rate, bits = fmt
    if ch < 1:
        raise WaveFormatError("%s: no channels" % path)
    if (tag, bits) not in ((1, 8), (1, 16), (1, 24), (1, 32), (3, 32), (3, 64)) and (tag, bits) not in _G711_KIND:
        raise WaveFormatError("%s: unsupported WAVE format tag %d with %d bits" % (path, tag, bits))
    return dict(tag=tag, bits=bits, channels=ch, rate=rate, frames=nbytes // ((bits // 8) * ch))


def file_groups(paths, max_bytes):
    """Consecutive files in groups of at most max_bytes of mono f32 samples at their native rates (a file larger than that is
    a group of its own), from the chunk headers alone: 4 bytes per frame wave_info counts, the frames the loader decodes.  A
    file that wave_info refuses counts 0 bytes: the loader reports what is wrong with it."""
    sizes = []
    for path in paths:
        try:
            sizes.append(4 * wave_info(path)["frames"])
        except (OSError, WaveFormatError):
            sizes.append(0)
    return ragged.byte_groups(sizes, max_bytes)


def load_device(path, sr=22050, mono=True, offset=0.0, duration=None, res_type="kaiser_best", device="cuda"):
    """`librosa.load` with the result left in HBM: (y f32 GPU tensor, sr).  mono=False is not on the
    reference's path (every call site takes the default) and raises."""
    if not mono:
        raise NotImplementedError("load(mono=False): the reference only loads mono (M1/dataset.py:226)")
    if not torch.cuda.is_available():
        raise RuntimeError("sos_amd.audio_io needs an MI355X: there is no CPU fallback")
    arr, kind, sr_native = read_wave(path)
    if offset:
        arr = arr[int(offset * sr_native):]
    if duration is not None:
        arr = arr[:int(duration * sr_native)]
    if arr.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float32, device=device), (sr_native if sr is None else sr)
    pcm = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    y = pcm_to_mono_device(pcm, kind)
    if sr is not None and sr != sr_native:
        y = resample_device(y, sr_native, sr, res_type)
    else:
        sr = sr_native
    return y, sr


def load_batch_device(paths, sr=22050, mono=True, offset=0.0, duration=None, res_type="kaiser_best", device="cuda"):
    """load_device of every file of a list: (ys, srs), one f32 GPU tensor and one rate per file, each bit for bit
    load_device(path).  Every file is parsed on the host; files that share (sample format, channel count) go up in one
    copy of their concatenated frames and through one sos_pcm_to_mono_f32 launch, files that share a native rate other
    than `sr` through one sos_resample_batch_f32 launch: the number of launches and copies follows the number of distinct
    formats and rates, not the number of files."""
    if not mono:
        raise NotImplementedError("load(mono=False): the reference only loads mono (M1/dataset.py:226)")
    if not torch.cuda.is_available():
        raise RuntimeError("sos_amd.audio_io needs an MI355X: there is no CPU fallback")
    paths = list(paths)
    ys, rates, by_format = [None] * len(paths), [], {}
    for i, path in enumerate(paths):
        arr, kind, sr_native = read_wave(path)
        if offset:
            arr = arr[int(offset * sr_native):]
        if duration is not None:
            arr = arr[:int(duration * sr_native)]
        rates.append(sr_native)
        if arr.shape[0] == 0:
            ys[i] = torch.zeros(0, dtype=torch.float32, device=device)
        else:
            by_format.setdefault((kind, arr.shape[1]), []).append((i, arr))
    for (kind, _), group in by_format.items():
        pcm = torch.from_numpy(np.concatenate([arr for _, arr in group])).to(device)
        mono_all = pcm_to_mono_device(pcm, kind)          # per frame: the concatenation needs no table
        for (i, _), y in zip(group, ragged.split(mono_all, [arr.shape[0] for _, arr in group])):
            ys[i] = y
    if sr is None:
        return ys, rates
    by_rate = {}
    for i, r in enumerate(rates):
        if r != sr and ys[i].numel():
            by_rate.setdefault(r, []).append(i)
    for r, idx in by_rate.items():
        for i, y in zip(idx, resample_batch_device([ys[i] for i in idx], r, sr, res_type)):
            ys[i] = y
    return ys, [sr] * len(paths)


# ------------------------------------------------------------------------------------ channel planes (csrc/pcm_io.hip)
# encode formats: name -> (SOS_ENC_* of include/sos_hip.h, bytes per element, WAVE format tag, stored bits)
ENCODINGS = {"s16": (0, 2, 1, 16), "s32": (1, 4, 1, 32), "f32": (2, 4, 3, 32), "u8": (3, 1, 1, 8), "s24": (4, 3, 1, 24)}
# G.711, one code byte per sample: name -> (SOS_G711_* of include/sos_hip.h = the WAVE format tag, bytes per element, tag, bits)
G711 = {"alaw": (6, 1, 6, 8), "ulaw": (7, 1, 7, 8)}
_G711_KIND = {(v[2], v[3]): k for k, v in G711.items()}


def _back_to_back(tensors):
    """One 1-D tensor holding the elements of `tensors` in order: a view when they already lie back to back in one buffer (what
    ragged.split, resample_batch_device and denoise_long return), their concatenation otherwise."""
    first = tensors[0]
    at, base = first.storage_offset(), first.untyped_storage().data_ptr()
    for t in tensors:
        if not t.is_contiguous() or t.untyped_storage().data_ptr() != base or t.storage_offset() != at or t.dtype != first.dtype:
            return torch.cat([t.reshape(-1) for t in tensors])
        at += t.numel()
    return first.as_strided((at - first.storage_offset(),), (1,), first.storage_offset())


def planes_of(channels):
    """The equally long 1-D f32 GPU tensors of one file's channels as one (channels, n) tensor (a view if they lie back to back)."""
    return _back_to_back(list(channels)).view(len(channels), -1)


def decode_planes_batch_device(arrs, kinds, device="cuda"):
    """arrs: one (frames, channels) host array per file as read_wave returns it, kinds: its sample format ('s16', 's32', 'f32',
    'u8', or 'alaw' / 'ulaw' for uint8 G.711 codes); channel counts (1 .. 64) may differ from file to file.  -> one (channels,
    frames) f32 GPU tensor per file, views into ONE buffer, every value bit for bit what pcm_to_mono_device gives a one-channel
    file (sample / 2^(bits-1); G.711: the code's level / 2^15).  Files that share a sample format go up in one copy of their
    concatenated frames and through one sos_pcm_planes_batch_f32 / sos_g711_planes_batch_f32 launch (per 65535 files).
    ValueError before any launch: an unknown format, a file that is not 2-D or has 0 or more than 64 channels."""
    arrs, kinds = list(arrs), list(kinds)
    if len(arrs) != len(kinds):
        raise ValueError("decode_planes_batch_device: one kind per array (%d arrays, %d kinds)" % (len(arrs), len(kinds)))
    by_kind = {}
    for i, (a, k) in enumerate(zip(arrs, kinds)):
        if k not in _FMT and k not in G711:
            raise ValueError("decode_planes_batch_device: file %d has the unsupported sample format %r" % (i, k))
        if a.ndim != 2 or not 1 <= a.shape[1] <= 64:
            raise ValueError("decode_planes_batch_device: file %d must be (frames, 1 .. 64 channels), got shape %s" % (i, a.shape))
        if a.shape[0]:
            by_kind.setdefault(k, []).append(i)
    if not torch.cuda.is_available():
        raise RuntimeError("sos_amd.audio_io needs an MI355X: there is no CPU fallback")
    sizes = np.asarray([a.size for a in arrs], dtype=np.int64)
    order = [i for idx in by_kind.values() for i in idx]
    out = torch.empty(int(sizes.sum()), dtype=torch.float32, device=device)
    where = dict(zip(order, ragged.offsets(sizes[order]).tolist()))
    h = L.lib()
    for k, idx in by_kind.items():
        name = "sos_g711_planes_batch_f32" if k in G711 else "sos_pcm_planes_batch_f32"
        entry, code = getattr(h, name), G711[k][0] if k in G711 else _FMT[k]
        pcm = torch.from_numpy(np.concatenate([arrs[i].reshape(-1) for i in idx])).to(device)
        off = ragged.offsets(sizes[idx])
        for c0 in range(0, len(idx), ragged.MAX_CLIPS):
            sel = idx[c0:c0 + ragged.MAX_CLIPS]
            o0 = where[sel[0]]
            tab = np.asarray([[off[c0 + j] - off[c0], arrs[i].shape[0], arrs[i].shape[1], where[i] - o0] for j, i in enumerate(sel)],
                             dtype=np.int64)
            tab_dev = torch.from_numpy(tab).to(device)
            L.check(entry(L.ptr(pcm[int(off[c0]):]), code, L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), len(sel), L.ptr(out[o0:]),
                          L.stream_ptr()), name)
    return [out[where[i]:where[i] + a.size].view(a.shape[1], a.shape[0]) if a.shape[0]
            else torch.zeros((a.shape[1], 0), dtype=torch.float32, device=device) for i, a in enumerate(arrs)]


def load_channels_batch_device(paths, sr=None, res_type="kaiser_best", device="cuda"):
    """Every channel of every file of a list, nothing mixed down: (ys, srs, infos) with ys[i] a (channels, n) f32 GPU tensor (a
    view into one buffer), srs[i] its rate and infos[i] = read_wave_info's dict(tag, bits, channels, rate, frames) of the SOURCE
    (bits as stored).  Every file is parsed on the host; files that share a sample format go up in one copy and through one
    decode launch (decode_planes_batch_device); with `sr`, all channels of all files that share a native rate other than `sr` go
    through ONE resample_batch_device call, channel c of file i bit for bit resample_device(ys[i][c]).  sr=None keeps the native
    rates.  (load_device / load_batch_device with mono=False keep raising: they are librosa's signatures.)"""
    paths = list(paths)
    parsed = [read_wave_info(p) for p in paths]
    ys = decode_planes_batch_device([p[0] for p in parsed], [p[1] for p in parsed], device)
    rates, infos = [p[2] for p in parsed], [p[3] for p in parsed]
    if sr is None:
        return ys, rates, infos
    by_rate = {}
    for i, r in enumerate(rates):
        if r != sr and ys[i].shape[1]:
            by_rate.setdefault(r, []).append(i)
    for r, idx in by_rate.items():
        outs = resample_batch_device([ys[i][c] for i in idx for c in range(ys[i].shape[0])], r, sr, res_type)
        k = 0
        for i in idx:
            ch = ys[i].shape[0]
            ys[i] = planes_of(outs[k:k + ch])
            k += ch
    return ys, [sr] * len(paths), infos


def encode_batch_device(planes, fmt, frames=None):
    """planes: one (channels, n) f32 GPU tensor per file; fmt: 's16', 's24' (packed, 3 bytes little-endian), 's32', 'u8' or
    'f32'; frames: samples per channel to write per file (default: n).  -> (data, offsets, clipped): one uint8 GPU tensor with
    the files' interleaved [frames][channels] data back to back, the host int64 byte offsets (files + 1 entries) and an int64
    GPU tensor of per-file counts, from ONE sos_pcm_encode_batch launch (per 65535 files).  Per sample: the plane's value below
    n and 0 from there to `frames` (crop / zero-fill happen in the kernel); f32 copies the bits; otherwise q = rint(x * S) half
    to even in double with S = 2^(bits-1), NaN -> 0, saturated to [-S, S - 1]; u8 stores q + 128.  clipped[f] counts the samples
    that were NaN or changed by saturation (+-inf included).  NO dither is applied (out of scope): quantisation error is
    correlated with the signal, as with soundfile's and scipy's integer writers.  Float64 restatement: tests/pcm_reference.py.
    'alaw' / 'ulaw' (G.711, one code byte per sample, ONE sos_g711_encode_batch launch): the 's16' value q, counted as 's16'
    counts it, through the reference compressor (include/sos_hip.h; it drops the low bits of q, as audioop, libsndfile and sox
    do); the zero-fill is the code of silence, 0xD5 / 0xFF.  Restatement: tests/g711_reference.py."""
    planes = list(planes)
    if fmt not in ENCODINGS and fmt not in G711:
        raise ValueError("encode_batch_device: unsupported sample format %r (one of %s)"
                         % (fmt, ", ".join(sorted(ENCODINGS) + sorted(G711))))
    code, width = (G711[fmt] if fmt in G711 else ENCODINGS[fmt])[:2]
    name = "sos_g711_encode_batch" if fmt in G711 else "sos_pcm_encode_batch"
    for i, p in enumerate(planes):
        if not torch.is_tensor(p) or p.dim() != 2 or p.dtype != torch.float32 or not 1 <= p.shape[0] <= 64:
            raise ValueError("encode_batch_device: file %d must be a (1 .. 64 channels, n) float32 tensor" % i)
    L.require_cuda(*planes)
    frames = [int(p.shape[1]) for p in planes] if frames is None else [int(f) for f in frames]
    if len(frames) != len(planes) or min(frames, default=0) < 0:
        raise ValueError("encode_batch_device: frames holds one non-negative count per file")
    chans = np.asarray([p.shape[0] for p in planes], dtype=np.int64)
    avail = np.asarray([p.shape[1] for p in planes], dtype=np.int64)
    elems = chans * np.asarray(frames, dtype=np.int64)
    offsets = np.concatenate([ragged.offsets(elems), [elems.sum()]]).astype(np.int64) * width
    if not planes:
        return torch.zeros(0, dtype=torch.uint8, device="cuda"), offsets, torch.zeros(0, dtype=torch.int64, device="cuda")
    device = planes[0].device
    flat = _back_to_back(planes) if int((chans * avail).sum()) else torch.zeros(1, dtype=torch.float32, device=device)
    src = ragged.offsets(chans * avail)
    data = torch.empty(max(int(offsets[-1]), 1), dtype=torch.uint8, device=device)
    clipped = torch.empty(len(planes), dtype=torch.int64, device=device)
    h = L.lib()
    for c0 in range(0, len(planes), ragged.MAX_CLIPS):
        c1 = min(c0 + ragged.MAX_CLIPS, len(planes))
        e0 = int(offsets[c0]) // width
        tab = np.ascontiguousarray(np.stack([src[c0:c1] - src[c0], avail[c0:c1], chans[c0:c1], np.asarray(frames[c0:c1], dtype=np.int64),
                                             offsets[c0:c1] // width - e0], axis=1), dtype=np.int64)
        tab_dev = torch.from_numpy(tab).to(device)
        L.check(getattr(h, name)(L.ptr(flat[int(src[c0]):]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0, code,
                                 L.ptr(data[e0 * width:]), L.ptr(clipped[c0:]), L.stream_ptr()), name)
    return data[:int(offsets[-1])], offsets, clipped


def planes_together(planes):
    """The (channels, n) f32 GPU tensors of a group of files as views into ONE buffer, files back to back: the tensors
    themselves where they already lie so, views into one copy otherwise."""
    planes = list(planes)
    if not planes:
        return planes
    flat = _back_to_back(planes)
    if flat.untyped_storage().data_ptr() == planes[0].untyped_storage().data_ptr():
        return planes
    return [v.view(p.shape) for v, p in zip(ragged.split(flat, [p.numel() for p in planes]), planes)]


def loudness_gain_batch_device(planes, stats, target, peak_ceiling_db=-1.0, frames=None):
    """Brings every file of a group to a target loudness, IN PLACE and in one sos_loudness_gain_batch_f32 launch (per 65535
    files), without a wait.  planes: one (channels, n) f32 GPU tensor per file; stats: what metrics.loudness_batch returned for
    them (its dict, or the f64 [files][4] rows {L, peak, ..}); target: LUFS, one float for all files or an f64 GPU tensor of one
    per file (the 'source' mode hands over the loudness it measured, still on the device); peak_ceiling_db: dBFS (<= 0) the
    SAMPLE peak of the scaled file may reach; frames: samples per channel to scale per file (default n; what lies past them
    keeps its value).  Per file, in float64, g = min(10^((target - L) / 20), 10^(ceiling / 20) / peak), stored as float32; g = 1
    where L is -inf (no block passed the gates), the peak is 0 or the target is not finite; out = x * g, one float32 multiply.
    -> (gains f32 [files], limited bool [files]: the ceiling bound the gain), on the device.  Float64 restatement:
    tests/loudness_reference.py."""
    planes = list(planes)
    for i, p in enumerate(planes):
        if not torch.is_tensor(p) or p.dim() != 2 or p.dtype != torch.float32 or not 1 <= p.shape[0] <= 64:
            raise ValueError("loudness_gain_batch_device: file %d must be a (1 .. 64 channels, n) float32 tensor" % i)
    rows = stats["rows"] if isinstance(stats, dict) else stats
    if not torch.is_tensor(rows) or rows.dtype != torch.float64 or tuple(rows.shape) != (len(planes), 4):
        raise ValueError("loudness_gain_batch_device: stats holds one float64 row of 4 per file (metrics.loudness_batch)")
    if torch.is_tensor(target):
        if target.dtype != torch.float64 or tuple(target.shape) != (len(planes),):
            raise ValueError("loudness_gain_batch_device: a target tensor holds one float64 per file")
    elif not np.isfinite(float(target)):
        raise ValueError("loudness_gain_batch_device: the target is a finite number of LUFS, got %r" % (target,))
    if not float(peak_ceiling_db) <= 0.0:
        raise ValueError("loudness_gain_batch_device: the ceiling is at most 0 dBFS, got %r" % (peak_ceiling_db,))
    frames = [int(p.shape[1]) for p in planes] if frames is None else [int(f) for f in frames]
    if len(frames) != len(planes) or min(frames, default=0) < 0:
        raise ValueError("loudness_gain_batch_device: frames holds one non-negative count per file")
    L.require_cuda(rows, *planes)
    if not planes:
        return torch.zeros(0, dtype=torch.float32, device="cuda"), torch.zeros(0, dtype=torch.bool, device="cuda")
    device = planes[0].device
    if torch.is_tensor(target):
        L.require_cuda(target)
        targets = target.contiguous()
    else:
        targets = torch.full((len(planes),), float(target), dtype=torch.float64, device=device)
    rows = rows.contiguous()
    chans = np.asarray([p.shape[0] for p in planes], dtype=np.int64)
    avail = np.asarray([p.shape[1] for p in planes], dtype=np.int64)
    together = planes_together(planes) if int((chans * avail).sum()) else planes
    flat = _back_to_back(together) if int((chans * avail).sum()) else torch.zeros(1, dtype=torch.float32, device=device)
    src = ragged.offsets(chans * avail)
    gains = torch.empty(len(planes), dtype=torch.float32, device=device)
    limited = torch.empty(len(planes), dtype=torch.int32, device=device)
    h = L.lib()
    for c0 in range(0, len(planes), ragged.MAX_CLIPS):
        c1 = min(c0 + ragged.MAX_CLIPS, len(planes))
        tab = np.zeros((c1 - c0, 8), dtype=np.int64)
        tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3] = src[c0:c1] - src[c0], avail[c0:c1], chans[c0:c1], frames[c0:c1]
        tab_dev = torch.from_numpy(tab).to(device)
        L.check(h.sos_loudness_gain_batch_f32(L.ptr(flat[int(src[c0]):]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0,
                                              L.ptr(rows[c0:]), L.ptr(targets[c0:]), float(peak_ceiling_db), L.ptr(gains[c0:]),
                                              L.ptr(limited[c0:]), L.stream_ptr()), "sos_loudness_gain_batch_f32")
    for p, t in zip(planes, together):
        if t is not p:                                  # the planes lay apart: the launch scaled their copy
            p.copy_(t)
    return gains, limited.bool()


def g711_decode_device(codes, law):
    """One chunk of a G.711 leg (a packet's payload): codes 1-D uint8 (GPU tensor, numpy array or bytes), law 'alaw' / 'ulaw' ->
    1-D f32 GPU tensor, what decode_planes_batch_device gives a one-channel file.  The rule has no state: the chunks of a signal
    decode to the chunks of its decode."""
    if law not in G711:
        raise ValueError("g711_decode_device: unknown law %r (one of %s)" % (law, ", ".join(sorted(G711))))
    if torch.is_tensor(codes):
        if codes.dim() != 1 or codes.dtype != torch.uint8:
            raise ValueError("g711_decode_device expects 1-D uint8 codes")
        L.require_cuda(codes)
        if not codes.numel():
            return torch.zeros(0, dtype=torch.float32, device=codes.device)
        return pcm_to_mono_device(codes.view(-1, 1), law)         # one channel: the planes kernel's bits
    arr = np.frombuffer(codes, dtype=np.uint8) if isinstance(codes, (bytes, bytearray, memoryview)) else np.asarray(codes)
    if arr.ndim != 1 or arr.dtype != np.uint8:
        raise ValueError("g711_decode_device expects 1-D uint8 codes")
    return decode_planes_batch_device([arr.reshape(-1, 1)], [law])[0][0]


def g711_encode_device(x, law):
    """One chunk of a leg's output: x 1-D f32 GPU tensor -> (1-D uint8 GPU tensor of codes, clipped: int64 GPU tensor of one
    count), encode_batch_device([x[None]], law).  No state: the chunks of a signal encode to the chunks of its encode."""
    if law not in G711:
        raise ValueError("g711_encode_device: unknown law %r (one of %s)" % (law, ", ".join(sorted(G711))))
    if not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.float32:
        raise ValueError("g711_encode_device expects a 1-D float32 tensor")
    data, _, clipped = encode_batch_device([x.view(1, -1)], law)
    return data, clipped


# ------------------------------------------------------------------------------------ the band above SR / 2 (csrc/band_merge.hip)
def _flat_f32(tensors, device):
    """_back_to_back of 1-D f32 tensors of which some (or all) may be empty: never a null pointer."""
    full = [t for t in tensors if t.numel()]
    return _back_to_back(full) if full else torch.zeros(1, dtype=torch.float32, device=device)


def _check_low_pairs(who, lows_in, lows_out, min_out):
    if len(lows_in) != len(lows_out):
        raise ValueError("%s: one output per input of the networks (%d inputs, %d outputs)" % (who, len(lows_in), len(lows_out)))
    for i, (a, b) in enumerate(zip(lows_in, lows_out)):
        for t in (a, b):
            if not torch.is_tensor(t) or t.dim() != 1 or t.dtype != torch.float32:
                raise ValueError("%s: clip %d: expects 1-D float32 tensors" % (who, i))
        if a.numel() < 1 or not min_out <= b.numel() <= a.numel():
            raise ValueError("%s: clip %d: the networks' output has %d samples for an input of %d (%d .. the input's length, and "
                             "an input of at least 1)" % (who, i, b.numel(), a.numel(), min_out))


def band_gains_batch_device(lows_in, lows_out, hop=transform.HOP_LENGTH, smooth_frames=2):
    """How much of each hop frame the networks kept: lows_in[i] = a, the m_i samples they were given, lows_out[i] = b, the m'_i <=
    m_i samples they returned (1-D f32 GPU tensors) -> one f32 GPU tensor s of J_i = ceil(m_i / hop) gains per clip, views into
    one buffer, from ONE sos_band_gain_batch_f32 launch (per 65535 clips).  Frame j covers samples [j hop, (j + 1) hop) cut at m;
    r[j] = 1 if sum a^2 == 0 else min(1, sqrt(sum b^2 / sum a^2)) in float64, b reading zero from m' on (so the last partial frame
    has r = 0); s[j] = the float64 mean of r[j - smooth_frames .. j + smooth_frames] cut at the clip's ends, stored as f32.
    Float64 restatement: tests/band_reference.py.
    ValueError before any launch: lists of different lengths, tensors that are not 1-D float32, m < 1, m' > m, hop < 1,
    smooth_frames outside 0 .. 16.  RuntimeError for CPU tensors: there is no fallback."""
    lows_in, lows_out, hop = list(lows_in), list(lows_out), int(hop)
    _check_low_pairs("band_gains_batch_device", lows_in, lows_out, 0)
    if hop < 1 or not 0 <= int(smooth_frames) <= 16:
        raise ValueError("band_gains_batch_device: hop is at least 1 (got %d) and smooth_frames within 0 .. 16 (got %s)"
                         % (hop, smooth_frames))
    L.require_cuda(*lows_in, *lows_out)
    if not lows_in:
        return []
    device = lows_in[0].device
    m = np.asarray([a.numel() for a in lows_in], dtype=np.int64)
    mp = np.asarray([b.numel() for b in lows_out], dtype=np.int64)
    J = -(-m // hop)
    a_off, b_off, g_off = ragged.offsets(m), ragged.offsets(mp), ragged.offsets(J)
    a, b = _flat_f32(lows_in, device), _flat_f32(lows_out, device)
    gains = torch.empty(int(J.sum()), dtype=torch.float32, device=device)
    h = L.lib()
    for c0 in range(0, len(lows_in), ragged.MAX_CLIPS):
        c1 = min(c0 + ragged.MAX_CLIPS, len(lows_in))
        a0, b0, g0 = int(a_off[c0]), int(b_off[c0]), int(g_off[c0])
        tab = np.ascontiguousarray(np.stack([a_off[c0:c1] - a0, m[c0:c1], b_off[c0:c1] - b0, mp[c0:c1], g_off[c0:c1] - g0, J[c0:c1]]),
                                   dtype=np.int64)
        tab_dev = torch.from_numpy(tab).to(device)
        L.check(h.sos_band_gain_batch_f32(L.ptr(a[a0:]), L.ptr(b[min(b0, b.numel() - 1):]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p),
                                          c1 - c0, hop, int(smooth_frames), L.ptr(gains[g0:]), L.stream_ptr()), "sos_band_gain_batch_f32")
    return ragged.split(gains, J)


def resample_merge_batch_device(natives, lows_in, lows_out, orig_sr, target_sr, gains=None, res_type="kaiser_best", hop=transform.HOP_LENGTH):
    """Puts back what a chain at the lower rate orig_sr never saw of signals at target_sr > orig_sr.  Per clip: natives[i] = x
    (n frames at target_sr), lows_in[i] = a = x resampled to orig_sr (m = ceil(n * orig_sr / target_sr) samples: resample_batch_
    device's), lows_out[i] = b, the chain's output for a (1 <= m' <= m samples), all 1-D f32 GPU tensors; U = resample_device
    from orig_sr to target_sr (zero from (int64)(len * ratio) on).  ->
        out[t] = fmaf(g[t], x[t] - U(a)[t], U(b)[t])        0 <= t < n
    one (n,) f32 GPU tensor per clip, back to back in one buffer (planes_of yields views), from ONE
    sos_resample_merge_batch_f32 launch (per 65535 clips) that evaluates both resamplings with resample_device's bits.
    gains=None: g = 1 -- the band above orig_sr / 2 passes untouched; otherwise gains[i] = band_gains_batch_device's s for the
    clip (ceil(m / hop) values), interpolated linearly between frame centres.  Float64 restatement: tests/band_reference.py.
    ValueError before any launch: lists of different lengths, tensors that are not 1-D float32, m' > m or < 1, target_sr <=
    orig_sr, a clip whose a does not cover its n frames, a gains tensor of the wrong length, an unsupported res_type.
    RuntimeError for CPU tensors: there is no fallback."""
    natives, lows_in, lows_out, hop = list(natives), list(lows_in), list(lows_out), int(hop)
    who = "resample_merge_batch_device"
    if not target_sr > orig_sr:
        raise ValueError("%s: target_sr (%s) must exceed orig_sr (%s): there is no band to put back otherwise" % (who, target_sr, orig_sr))
    if res_type != "kaiser_best":
        raise ValueError("res_type %r is not supported (the reference uses librosa's default 'kaiser_best')" % (res_type,))
    if len(natives) != len(lows_in) or (gains is not None and len(gains) != len(natives)) or hop < 1:
        raise ValueError("%s: one native clip%s per low-rate clip (%d natives, %d low-rate inputs%s) and hop at least 1"
                         % (who, " and one gains tensor" if gains is not None else "", len(natives), len(lows_in),
                            ", %d gains" % len(gains) if gains is not None else ""))
    _check_low_pairs(who, lows_in, lows_out, 1)
    ratio = float(target_sr) / orig_sr
    gains = None if gains is None else list(gains)
    for i, x in enumerate(natives):
        if not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.float32:
            raise ValueError("%s: clip %d: expects 1-D float32 tensors" % (who, i))
        m = lows_in[i].numel()
        if x.numel() < 1 or int(m * ratio) < x.numel():
            raise ValueError("%s: clip %d: %d frames at %s Hz are not covered by %d samples at %s Hz (they give %d)"
                             % (who, i, x.numel(), target_sr, m, orig_sr, int(m * ratio)))
        if gains is not None:
            g = gains[i]
            if not torch.is_tensor(g) or g.dim() != 1 or g.dtype != torch.float32 or g.numel() != -(-m // hop):
                raise ValueError("%s: clip %d: gains must be a 1-D float32 tensor of ceil(%d / %d) = %d values"
                                 % (who, i, m, hop, -(-m // hop)))
    L.require_cuda(*natives, *lows_in, *lows_out, *(gains or []))
    if not natives:
        return []
    device = natives[0].device
    win, num_table = _filter_on(device, ratio, res_type)
    n = np.asarray([x.numel() for x in natives], dtype=np.int64)
    m = np.asarray([a.numel() for a in lows_in], dtype=np.int64)
    mp = np.asarray([b.numel() for b in lows_out], dtype=np.int64)
    J = -(-m // hop)
    x_off, a_off, b_off, g_off = ragged.offsets(n), ragged.offsets(m), ragged.offsets(mp), ragged.offsets(J)
    x, a, b = _back_to_back(natives), _back_to_back(lows_in), _back_to_back(lows_out)
    s = _back_to_back(gains) if gains is not None else None
    out = torch.empty(int(n.sum()), dtype=torch.float32, device=device)
    h = L.lib()
    for c0 in range(0, len(natives), ragged.MAX_CLIPS):
        c1 = min(c0 + ragged.MAX_CLIPS, len(natives))
        x0, a0, b0, g0 = int(x_off[c0]), int(a_off[c0]), int(b_off[c0]), int(g_off[c0])
        tiles = -(-n[c0:c1] // L.RESAMPLE_CHUNK)
        tab = np.ascontiguousarray(np.stack([x_off[c0:c1] - x0, n[c0:c1], a_off[c0:c1] - a0, m[c0:c1], b_off[c0:c1] - b0, mp[c0:c1],
                                             g_off[c0:c1] - g0, J[c0:c1], ragged.offsets(tiles)]), dtype=np.int64)
        tab_dev = torch.from_numpy(tab).to(device)
        L.check(h.sos_resample_merge_batch_f32(L.ptr(x[x0:]), L.ptr(a[a0:]), L.ptr(b[b0:]), L.ptr(s[g0:]) if s is not None else None,
                                               L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0, ratio, L.ptr(win), win.numel(),
                                               num_table, hop, L.ptr(out[x0:]), L.stream_ptr()), "sos_resample_merge_batch_f32")
    return ragged.split(out, n)


def load_batch(paths, sr=22050, mono=True, offset=0.0, duration=None, dtype=np.float32, res_type="kaiser_best"):
    """load of every file of a list, through load_batch_device: (list of ndarrays, list of rates)."""
    ys, srs = load_batch_device(paths, sr, mono, offset, duration, res_type)
    return ragged.download(ys, dtype), srs


def load(path, sr=22050, mono=True, offset=0.0, duration=None, dtype=np.float32, res_type="kaiser_best"):
    """Drop-in for `librosa.load` (librosa 0.7.1 core/audio.py) on WAVE files: (y ndarray, sr)."""
    y, sr = load_device(path, sr, mono, offset, duration, res_type)
    return np.ascontiguousarray(y.cpu().numpy(), dtype=dtype), sr


def to_mono(y):
    """librosa.to_mono: (channels, n) -> (n,) mean; 1-D passes through."""
    y = np.asarray(y)
    if y.ndim == 1:
        return y
    pcm = torch.from_numpy(np.ascontiguousarray(y.T, dtype=np.float32)).cuda()
    return pcm_to_mono_device(pcm, "f32").cpu().numpy().astype(y.dtype, copy=False)


def resample(y, orig_sr, target_sr, res_type="kaiser_best", fix=True, scale=False):
    """librosa.resample (1-D): numpy in -> numpy out."""
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("resample expects a 1-D signal")
    if orig_sr == target_sr:
        return y
    ratio = float(target_sr) / orig_sr
    out = resample_device(torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda(), orig_sr, target_sr,
                          res_type, fix).cpu().numpy()
    if scale:
        out = out / np.sqrt(ratio)
    return np.ascontiguousarray(out, dtype=y.dtype if np.issubdtype(y.dtype, np.floating) else np.float32)


def resample_batch(ys, orig_sr, target_sr, res_type="kaiser_best", fix=True, scale=False):
    """resample of every signal of a list (1-D, any lengths): numpy in -> numpy out, one upload and one download for the
    whole batch."""
    ys = [np.asarray(y) for y in ys]
    for y in ys:
        if y.ndim != 1:
            raise ValueError("resample expects a 1-D signal")
    if orig_sr == target_sr or not ys:
        return ys
    ratio = float(target_sr) / orig_sr
    flat = torch.from_numpy(np.concatenate([np.asarray(y, dtype=np.float32) for y in ys])).cuda()
    outs = ragged.download(resample_batch_device(ragged.split(flat, [len(y) for y in ys]), orig_sr, target_sr, res_type, fix),
                           np.float32)
    if scale:
        outs = [o / np.sqrt(ratio) for o in outs]
    return [np.ascontiguousarray(o, dtype=y.dtype if np.issubdtype(y.dtype, np.floating) else np.float32)
            for o, y in zip(outs, ys)]


def wave_bytes(y, sr):
    """Bytes of the file `scipy.io.wavfile.write(path, sr, y)` produces (what librosa.output.write_wav calls):
    int16/int32/uint8 -> PCM; float32/float64 -> IEEE float with an 18-byte fmt chunk and a `fact` chunk."""
    y = np.asarray(y)
    if y.ndim == 1:
        ch = 1
    elif y.ndim == 2:
        ch = y.shape[1]
    else:
        raise ValueError("wave data must be (n,) or (n, channels)")
    kind = y.dtype.kind
    if not (kind in "iu" and y.dtype.itemsize in (1, 2, 4, 8) or kind == "f" and y.dtype.itemsize in (4, 8)):
        raise ValueError("Unsupported data type '%s'" % y.dtype)
    if kind == "u" and y.dtype.itemsize != 1 or kind == "i" and y.dtype.itemsize == 1:
        raise ValueError("Unsupported data type '%s'" % y.dtype)
    tag = 3 if kind == "f" else 1
    bits = y.dtype.itemsize * 8
    data = np.ascontiguousarray(y).astype(y.dtype.newbyteorder("<"), copy=False).tobytes()
    return _riff(data, tag, ch, sr, bits, y.shape[0])


def _riff(data, tag, ch, sr, bits, frames):
    """The chunks around `data`: a 16-byte fmt chunk for PCM; an 18-byte one and a `fact` chunk with the frame count otherwise."""
    align = ch * (bits // 8)
    fmt = struct.pack("<HHIIHH", tag, ch, int(sr), int(sr) * align, align, bits)
    if tag != 1:
        fmt += b"\x00\x00"
    head = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if tag != 1:
        head += b"fact" + struct.pack("<II", 4, frames)
    if len(head) + len(data) + 12 > 0xFFFFFFFF:
        raise ValueError("Data exceeds wave file size limit")
    body = b"WAVE" + head + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def wave_container(data_bytes, tag, channels, rate, bits):
    """The RIFF/WAVE file around already-encoded interleaved data (encode_batch_device's bytes): tag 1 (PCM) with a 16-byte
    fmt chunk, tag 3 (IEEE float) with an 18-byte fmt chunk and a `fact` chunk, the chunks of wave_bytes -- for mono or
    interleaved f32 data, wave_container(y.tobytes(), 3, channels, sr, 32) == wave_bytes(y, sr).  Tags 6 / 7 (G.711 A-law /
    mu-law, 8 bits) get the chunks of every non-PCM format, the 18-byte fmt chunk and `fact`; like u8 data, an odd number of
    code bytes is followed by no pad byte."""
    data = bytes(data_bytes)
    if tag not in (1, 3) and (tag, bits) not in _G711_KIND or bits % 8 or bits < 8 or channels < 1:
        raise ValueError("wave_container: tag 1 (PCM), 3 (float) or 6 / 7 (G.711 A-law / mu-law, 8 bits), whole bytes per sample, "
                         "at least one channel")
    align = channels * (bits // 8)
    if len(data) % align:
        raise ValueError("wave_container: %d bytes are no whole number of %d-byte frames" % (len(data), align))
    return _riff(data, tag, channels, rate, bits, len(data) // align)


def write_wav(path, y, sr, norm=False):
    """librosa.output.write_wav (0.7.1 output.py): y mono (n,) or stereo (2, n); float data is written as
    32/64-bit float WAVE unchanged unless norm=True (peak-normalised to 1)."""
    if torch.is_tensor(y):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if not np.issubdtype(y.dtype, np.floating):
        raise ValueError("Audio data must be floating-point")          # librosa.util.valid_audio
    if y.ndim not in (1, 2) or not np.isfinite(y).all():
        raise ValueError("Audio buffer is not finite everywhere or has a bad shape")
    wav = y
    if norm:
        peak = np.max(np.abs(y)) if y.size else 0.0
        wav = y / peak if peak > np.finfo(y.dtype).tiny else y
    if wav.ndim > 1 and wav.shape[0] == 2:
        wav = wav.T
    with open(path, "wb") as fp:
        fp.write(wave_bytes(wav, sr))
