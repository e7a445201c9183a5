"""Mirror of the on-path pieces of the reference `tools.py` (M2/tools.py:217-303,340-362)."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from . import ragged


def bits_to_mask_batch(bits, ratio, n_samples, sig=None, clip_frames=None, clip_samples=None):
    """bits uint8 (B, n_frames) on the GPU (1 = non-silent) -> mask f32 (B, n_samples)
    (1 on silent samples) and, if `sig` is given, sig*mask (M2/predict.py:310,317).  clip_frames / clip_samples:
    optional int32 device (B,) each, ragged batch (clip b uses its own frame and sample counts)."""
    L.require_cuda(bits, sig)
    bits = bits.contiguous()
    if bits.dtype != torch.uint8 or bits.dim() != 2:
        raise ValueError("bits must be a uint8 (B, n_frames) tensor")
    B, nfr = bits.shape
    mask = torch.empty((B, n_samples), dtype=torch.float32, device=bits.device)
    masked = None
    if sig is not None:
        sig = sig.contiguous()
        if sig.shape != mask.shape or sig.dtype != torch.float32:
            raise ValueError("sig must be float32 (B, n_samples)")
        masked = torch.empty_like(sig)
    L.check(L.lib().sos_bits_to_mask(L.ptr(bits), B, nfr, float(ratio), n_samples, L.ptr(mask), L.ptr(sig),
                                     L.ptr(masked), L.ptr(clip_frames), L.ptr(clip_samples), L.stream_ptr()),
            "sos_bits_to_mask")
    return (mask, masked) if sig is not None else mask


def ragged_stage(flat, table, stride, bits=None, ratios=None):
    """A ragged group staged for the networks in one launch (sos_ragged_stage_f32).  flat: the clips back to back, f32 GPU
    tensor; table: host rows {sample offset, samples, bit offset, frames}, one per clip; bits: the clips' frame decisions back
    to back (uint8 GPU tensor, 1 = non-silent); ratios: samples per frame, one float per clip.
    -> (wave (B, stride), masked (B, stride), mask back to back like `flat`): the clip zero-filled to the stride, clip * mask
    likewise, and the sample mask (1 = silent), each clip's bit for bit bits_to_mask_batch of that clip alone at its ratio.
    Without `bits` only `wave` is computed and returned."""
    L.require_cuda(flat, bits)
    tab = ragged.host_table(table, 4)
    B = tab.shape[0]
    if flat.dim() != 1 or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("flat must be a contiguous 1-D float32 tensor")
    if flat.numel() < int(tab[:, 1].sum()):
        raise ValueError("the table names more samples than `flat` holds")
    wave = torch.empty((B, int(stride)), dtype=torch.float32, device=flat.device)
    d_tab = ragged.upload(tab, flat.device)
    masked = mask = rat = d_rat = None
    if bits is not None:
        if bits.dim() != 1 or bits.dtype != torch.uint8 or not bits.is_contiguous() or bits.numel() < int(tab[:, 3].sum()):
            raise ValueError("bits must be a contiguous 1-D uint8 tensor holding every frame of the table")
        rat = ragged.per_clip(ratios, B, "ratios")
        d_rat = ragged.upload(rat, flat.device)
        masked, mask = torch.empty_like(wave), torch.empty_like(flat)
    L.check(L.lib().sos_ragged_stage_f32(L.ptr(flat), L.ptr(d_tab), tab.ctypes.data, B, L.ptr(bits), L.ptr(d_rat),
                                         rat.ctypes.data if rat is not None else None, int(stride), L.ptr(wave), L.ptr(masked),
                                         L.ptr(mask), L.stream_ptr()), "sos_ragged_stage_f32")
    return (wave, masked, mask) if bits is not None else wave


def ragged_unpack(rows, table):
    """Padded rows f32 (R, stride) on the GPU + host table rows {row, valid samples, output offset} -> one 1-D f32 GPU tensor
    of sum(valid) samples, out[offset : offset + valid] = rows[row, :valid], in one launch (sos_ragged_unpack_f32): what a
    single download of a group's results needs."""
    L.require_cuda(rows)
    tab = ragged.host_table(table, 3)
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 (R, stride) tensor")
    out = torch.empty(int(tab[:, 1].sum()), dtype=torch.float32, device=rows.device)
    d_tab = ragged.upload(tab, rows.device)
    L.check(L.lib().sos_ragged_unpack_f32(L.ptr(rows), rows.shape[0], rows.shape[1], L.ptr(d_tab), tab.ctypes.data,
                                          tab.shape[0], L.ptr(out), L.stream_ptr()), "sos_ragged_unpack_f32")
    return out


WINDOW_COLS = 10                    # int64 per window of pipeline.window_plan (csrc/ragged_window.hip: RW_COLS)


def window_stage(x, table, stride):
    """Windows of a buffer as zero-filled rows in one launch (sos_window_stage_f32).  x: contiguous 1-D f32 GPU tensor; table:
    host rows of pipeline.window_plan, of which {source offset, samples} are read; windows may overlap and start on any sample.
    -> rows (windows, stride): rows[w, :samples] = x[source offset : source offset + samples], zero beyond."""
    L.require_cuda(x)
    tab = ragged.host_table(table, WINDOW_COLS)
    if x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous 1-D float32 tensor")
    rows = torch.empty((tab.shape[0], int(stride)), dtype=torch.float32, device=x.device)
    d_tab = ragged.upload(tab, x.device)
    L.check(L.lib().sos_window_stage_f32(L.ptr(x), x.numel(), L.ptr(d_tab), tab.ctypes.data, tab.shape[0], int(stride),
                                         L.ptr(rows), L.stream_ptr()), "sos_window_stage_f32")
    return rows


def window_stitch(rows, table, context):
    """The rows of overlapping windows cross-faded into their recordings' outputs in one launch (sos_window_stitch_f32).  rows:
    contiguous f32 (R, stride) GPU tensor; table: host rows of pipeline.window_plan, whose cores tile the outputs; context: half
    the width of the blend around an inner core boundary, in samples (0: a plain cut).
    -> one 1-D f32 GPU tensor, the recordings' outputs back to back (sum of the cores' lengths)."""
    L.require_cuda(rows)
    tab = ragged.host_table(table, WINDOW_COLS)
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 (R, stride) tensor")
    out = torch.empty(max(int((tab[:, 5] - tab[:, 4]).sum()), 0), dtype=torch.float32, device=rows.device)
    d_tab = ragged.upload(tab, rows.device)
    L.check(L.lib().sos_window_stitch_f32(L.ptr(rows), rows.shape[0], rows.shape[1], L.ptr(d_tab), tab.ctypes.data, tab.shape[0],
                                          int(context), L.ptr(out), L.stream_ptr()), "sos_window_stitch_f32")
    return out


MAX_PLANES = 8                      # signals one planes stitch takes (csrc/ragged_window.hip: RW_MAX_PLANES)


def window_stitch_planes(rows, table, context, recs=None, out_total=None):
    """window_stitch for several signals of the same plan in ONE launch (sos_window_stitch_planes_f32).  rows: contiguous f32
    (planes, R, stride) GPU tensor, 1 .. 8 planes; table, context: as window_stitch, and column 0 names each window's recording.
    Without `recs` the layout is plane-major: -> (planes, total), row q bit for bit window_stitch(rows[q], table, context).
    recs: host rows {base, pitch}, one per recording: sample p of plane q of recording r goes to element base_r + q * pitch_r + p
    of the flat buffer of `out_total` floats that is returned (file-major: the planes of a recording next to each other;
    pitch > the recording's length leaves a gap).  What no segment covers stays zero."""
    L.require_cuda(rows)
    tab = ragged.host_table(table, WINDOW_COLS)
    if rows.dim() != 3 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 (planes, R, stride) tensor")
    planes = rows.shape[0]
    if recs is None:
        if out_total is not None:
            raise ValueError("out_total goes with recs")
        nrec = int(tab[:, 0].max()) + 1
        if int(tab[:, 0].min()) < 0 or nrec > ragged.MAX_CLIPS:
            raise ValueError(f"the table names recordings outside 0 .. {ragged.MAX_CLIPS - 1}")
        lens = np.zeros(nrec, dtype=np.int64)
        np.add.at(lens, tab[:, 0], tab[:, 5] - tab[:, 4])
        total = max(int(lens.sum()), 0)
        rec = np.ascontiguousarray(np.stack([ragged.offsets(lens.tolist()), np.full(nrec, total, dtype=np.int64)], axis=1))
        out = torch.empty((planes, total), dtype=torch.float32, device=rows.device)          # the segments tile it
    else:
        if out_total is None:
            raise ValueError("recs needs out_total, the length of the flat buffer")
        rec = ragged.host_table(recs, 2)
        out = torch.zeros(max(int(out_total), 0), dtype=torch.float32, device=rows.device)
    d_tab, d_rec = ragged.upload(tab, rows.device), ragged.upload(rec, rows.device)
    L.check(L.lib().sos_window_stitch_planes_f32(L.ptr(rows), planes, rows.shape[1], rows.shape[2], L.ptr(d_tab), tab.ctypes.data,
                                                 tab.shape[0], int(context), L.ptr(d_rec), rec.ctypes.data, rec.shape[0],
                                                 out.numel(), L.ptr(out), L.stream_ptr()), "sos_window_stitch_planes_f32")
    return out


def window_frames_stitch(rows, table, win_frames, recs, ratios, core, context):
    """The windows' frame logits stitched into ONE logit stream per recording in one launch (sos_window_frames_stitch_f32; the
    rule and its float64 restatement: tests/frames_reference.py).  rows: contiguous f32 (R, stride) GPU tensor, a window's
    logits from column 0; table: host rows of pipeline.window_plan, of which {core start, core end, window start, row} are
    read; win_frames: the windows' numbers of logits; recs: host rows {frame offset in the output, frames, first window,
    windows}, one per recording; ratios: samples per frame, one value or one per recording; core, context: samples.
    -> one 1-D f32 GPU tensor, the recordings' logits back to back (sum of their frames)."""
    L.require_cuda(rows)
    tab, rec = ragged.host_table(table, WINDOW_COLS), ragged.host_table(recs, 4)
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 (R, stride) tensor")
    fr = np.ascontiguousarray(np.asarray(win_frames, dtype=np.int64).reshape(-1))
    if len(fr) != tab.shape[0]:
        raise ValueError("win_frames must hold one count per window of the table")
    rat = ragged.per_clip(ratios, rec.shape[0], "ratios")
    out = torch.empty(max(int(rec[:, 1].sum()), 0), dtype=torch.float32, device=rows.device)
    d_tab, d_fr, d_rec, d_rat = (ragged.upload(a, rows.device) for a in (tab, fr, rec, rat))
    L.check(L.lib().sos_window_frames_stitch_f32(L.ptr(rows), rows.shape[0], rows.shape[1], L.ptr(d_tab), tab.ctypes.data,
                                                 L.ptr(d_fr), fr.ctypes.data, tab.shape[0], L.ptr(d_rec), rec.ctypes.data,
                                                 L.ptr(d_rat), rat.ctypes.data, rec.shape[0], int(core), int(context), L.ptr(out),
                                                 L.stream_ptr()), "sos_window_frames_stitch_f32")
    return out


LINK_MODES = {"any": 0, "mean": 1}          # the `mode` of sos_window_frames_link_f32


def link_tables(link, frames):
    """The link tables of sos_window_frames_link_f32 (host only).  link: one group id per recording, None = a group of its
    own; recordings with equal ids are linked.  frames: the recordings' frame counts (members of a group must agree: the
    caller's check).  Groups stand in the order of their first member, members in recording order.
    -> (links int64 (groups, 4) = {frame offset of the group's stream, frames, first index into members, member count},
    members int64 (recordings,), group int64 (recordings,) = the group of each recording)."""
    index, rows, group = {}, [], []
    for r, g in enumerate(link):
        key = ("alone", r) if g is None else ("id", g)
        if key not in index:
            index[key] = len(rows)
            rows.append([])
        rows[index[key]].append(r)
        group.append(index[key])
    counts = [len(m) for m in rows]
    fr = [int(frames[m[0]]) for m in rows]
    links = np.stack([ragged.offsets(fr), np.asarray(fr, dtype=np.int64), ragged.offsets(counts),
                      np.asarray(counts, dtype=np.int64)], axis=1) if rows else np.zeros((0, 4), dtype=np.int64)
    return (np.ascontiguousarray(links, dtype=np.int64), np.asarray([r for m in rows for r in m], dtype=np.int64),
            np.asarray(group, dtype=np.int64))


def window_frames_link(rows, table, win_frames, recs, ratios, core, context, links, members, mode, threshold=0.5):
    """window_frames_stitch, the reduction over the recordings of a group and the decision in ONE launch
    (sos_window_frames_link_f32): one logit and one decision stream per GROUP.  rows .. context: as window_frames_stitch
    (the recs rows' frame offsets are not used); links: host rows {frame offset of the group's stream, frames, first index into
    members, member count}; members: recording indices; mode: 'any' (fmaxf in member order: a frame is speech if any member
    has speech) or 'mean' (sequential f32 sum in member order, one f32 divide); threshold: of the sigmoid, as threshold_bits.
    -> (logits f32, bits uint8), 1-D GPU tensors of sum(frames of the groups) elements, the groups' streams back to back."""
    L.require_cuda(rows)
    tab, rec, lk = ragged.host_table(table, WINDOW_COLS), ragged.host_table(recs, 4), ragged.host_table(links, 4)
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 (R, stride) tensor")
    fr = np.ascontiguousarray(np.asarray(win_frames, dtype=np.int64).reshape(-1))
    if len(fr) != tab.shape[0]:
        raise ValueError("win_frames must hold one count per window of the table")
    if mode not in LINK_MODES:
        raise ValueError(f"mode must be one of {sorted(LINK_MODES)}, got {mode!r}")
    mem = np.ascontiguousarray(np.asarray(members, dtype=np.int64).reshape(-1))
    if len(mem) < 1 or len(mem) != int(lk[:, 3].sum()):
        raise ValueError("members must hold one recording index per member the links count")
    rat = ragged.per_clip(ratios, rec.shape[0], "ratios")
    total = max(int(lk[:, 1].sum()), 0)
    logits = torch.empty(total, dtype=torch.float32, device=rows.device)
    bits = torch.empty(total, dtype=torch.uint8, device=rows.device)
    d_tab, d_fr, d_rec, d_rat, d_lk, d_mem = (ragged.upload(a, rows.device) for a in (tab, fr, rec, rat, lk, mem))
    L.check(L.lib().sos_window_frames_link_f32(L.ptr(rows), rows.shape[0], rows.shape[1], L.ptr(d_tab), tab.ctypes.data,
                                               L.ptr(d_fr), fr.ctypes.data, tab.shape[0], L.ptr(d_rec), rec.ctypes.data,
                                               L.ptr(d_rat), rat.ctypes.data, rec.shape[0], int(core), int(context), L.ptr(d_lk),
                                               lk.ctypes.data, L.ptr(d_mem), mem.ctypes.data, lk.shape[0], LINK_MODES[mode],
                                               float(threshold), L.ptr(logits), L.ptr(bits), L.stream_ptr()),
            "sos_window_frames_link_f32")
    return logits, bits


def window_stage_masked(flat, bits, clips, ratios, table, stride):
    """Windows of recordings staged together with their noise intervals in one launch (sos_window_stage_masked_f32).  flat: the
    recordings back to back, contiguous 1-D f32 GPU tensor; bits: their frame decisions back to back (uint8 GPU tensor, 1 =
    non-silent); clips: host rows {sample offset, samples, bit offset, frames}, one per recording, and ratios: samples per
    frame, one value or one per recording -- what ragged_stage takes; table: host rows of pipeline.window_plan, of which
    {recording, source offset, samples, window start} are read.
    -> (wave, masked), each (windows, stride): the window zero-filled to the stride, and window * mask likewise, the mask being
    the WHOLE recording's (ragged_stage's `mask` at the window's samples): bit for bit slices of ragged_stage's full-length
    rows, which are never made."""
    L.require_cuda(flat, bits)
    tab, clip = ragged.host_table(table, WINDOW_COLS), ragged.host_table(clips, 4)
    if flat.dim() != 1 or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("flat must be a contiguous 1-D float32 tensor")
    if flat.numel() < int(clip[:, 1].sum()):
        raise ValueError("the table names more samples than `flat` holds")
    if bits.dim() != 1 or bits.dtype != torch.uint8 or not bits.is_contiguous() or bits.numel() < int(clip[:, 3].sum()):
        raise ValueError("bits must be a contiguous 1-D uint8 tensor holding every frame of the table")
    rat = ragged.per_clip(ratios, clip.shape[0], "ratios")
    wave = torch.empty((tab.shape[0], int(stride)), dtype=torch.float32, device=flat.device)
    masked = torch.empty_like(wave)
    d_tab, d_clip, d_rat = (ragged.upload(a, flat.device) for a in (tab, clip, rat))
    L.check(L.lib().sos_window_stage_masked_f32(L.ptr(flat), L.ptr(bits), L.ptr(d_clip), clip.ctypes.data, L.ptr(d_rat),
                                                rat.ctypes.data, clip.shape[0], L.ptr(d_tab), tab.ctypes.data, tab.shape[0],
                                                int(stride), L.ptr(wave), L.ptr(masked), L.stream_ptr()),
            "sos_window_stage_masked_f32")
    return wave, masked


STREAM_PUSH_COLS, STREAM_STAGE_COLS, STREAM_STITCH_COLS = 4, 3, 8      # int64 per row (csrc/stream_window.hip: SW_*_COLS)
STREAM_HAS_PREV, STREAM_HAS_NEXT = 1, 2                                # flags of a stream_stitch row


def _stream_ring(ring):
    if ring.dim() != 2 or ring.dtype != torch.float32 or not ring.is_contiguous():
        raise ValueError("ring must be a contiguous float32 (slots, capacity) tensor")


def stream_push(flat, table, ring):
    """Chunks of live audio into their streams' rings in one launch (sos_stream_push_f32).  flat: the chunks back to back,
    contiguous 1-D f32 GPU tensor; table: host rows {slot, source offset, samples, stream position}, a slot at most once; ring:
    (slots, capacity) f32 GPU tensor, written in place: ring[slot, (position + j) % capacity] = flat[source offset + j]."""
    L.require_cuda(flat, ring)
    tab = ragged.host_table(table, STREAM_PUSH_COLS)
    _stream_ring(ring)
    if flat.dim() != 1 or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("flat must be a contiguous 1-D float32 tensor")
    d_tab = ragged.upload(tab, flat.device)
    L.check(L.lib().sos_stream_push_f32(L.ptr(flat), flat.numel(), L.ptr(d_tab), tab.ctypes.data, tab.shape[0], L.ptr(ring),
                                        ring.shape[0], ring.shape[1], L.stream_ptr()), "sos_stream_push_f32")


def stream_stage(ring, table, stride, out=None):
    """Windows of streams as zero-filled rows in one launch (sos_stream_stage_f32): window_stage out of the rings.  table: host
    rows {slot, stream position, samples}.  -> rows (windows, stride): rows[w, j] = ring[slot, (position + j) % capacity] for
    j < samples, zero beyond; `out`: a contiguous f32 (windows, stride) tensor to write instead (a captured graph's input)."""
    L.require_cuda(ring, out)
    tab = ragged.host_table(table, STREAM_STAGE_COLS)
    _stream_ring(ring)
    if out is None:
        out = torch.empty((tab.shape[0], int(stride)), dtype=torch.float32, device=ring.device)
    elif out.shape != (tab.shape[0], int(stride)) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 (windows, stride) tensor")
    d_tab = ragged.upload(tab, ring.device)
    L.check(L.lib().sos_stream_stage_f32(L.ptr(ring), ring.shape[0], ring.shape[1], L.ptr(d_tab), tab.ctypes.data, tab.shape[0],
                                         int(stride), L.ptr(out), L.stream_ptr()), "sos_stream_stage_f32")
    return out


def stream_stitch(rows, table, context, tail, out_stride=None):
    """What is final of each stream after one more window, in one launch (sos_stream_stitch_f32).  rows: contiguous f32
    (R, stride) GPU tensor; table: host rows {slot, row, window start, samples of the row, core start, core end, flags, parity};
    tail: (slots, 2, 2 context) f32 GPU tensor, the saved overlaps: half `parity` is read, half `parity ^ 1` written for a
    window with a next one (the caller then flips the slot's parity).
    -> (out (windows, out_stride), lengths): out[w, :lengths[w]] = the stream's samples [core start - context (core start
    without a previous window), core end - context (core end without a next one)), the first 2 context of them blended with
    the saved overlap exactly as window_stitch blends them.  out_stride: default the longest of `lengths`."""
    L.require_cuda(rows, tail)
    tab = ragged.host_table(table, STREAM_STITCH_COLS)
    context = int(context)
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 (R, stride) tensor")
    if tail.dim() != 3 or tuple(tail.shape[1:]) != (2, max(2 * context, 1)) or tail.dtype != torch.float32 or not tail.is_contiguous():
        raise ValueError("tail must be a contiguous float32 (slots, 2, 2 context) tensor (one column at context 0)")
    lo = tab[:, 4] - np.where(tab[:, 6] & STREAM_HAS_PREV, context, 0)
    hi = tab[:, 5] - np.where(tab[:, 6] & STREAM_HAS_NEXT, context, 0)
    lengths = np.maximum(hi - lo, 0)
    if out_stride is None:
        out_stride = max(int(lengths.max()), 1)
    out = torch.empty((tab.shape[0], int(out_stride)), dtype=torch.float32, device=rows.device)
    d_tab = ragged.upload(tab, rows.device)
    L.check(L.lib().sos_stream_stitch_f32(L.ptr(rows), rows.shape[0], rows.shape[1], L.ptr(d_tab), tab.ctypes.data, tab.shape[0],
                                          tail.shape[0], context, L.ptr(tail), L.ptr(out), int(out_stride), L.stream_ptr()),
            "sos_stream_stitch_f32")
    return out, lengths.tolist()


STREAM_RESAMPLE_COLS = 6                                               # int64 per row (csrc/stream_resample.hip: SRS_COLS)


def stream_resample(ring, table, ratio, win, num_table, out=None):
    """Outputs of streams resampled out of their rings in one launch (sos_stream_resample_f32).  ring: (slots, capacity) f32 GPU
    tensor as stream_push fills it; table: host rows {slot, t_lo, t_hi, n_in, n_valid, output offset}, a slot at most once: the
    outputs t_lo <= t < t_hi of the slot's stream, each as audio_io.resample_device computes it for a signal of n_in samples
    (zero from n_valid on), go to out[output offset ..]; ratio = target / orig; win, num_table: the filter's half window on the
    GPU, scaled by min(1, ratio), and its points per zero crossing (resampling.filter_on).
    -> out, a contiguous 1-D f32 GPU tensor: the one given, or a new one that ends with the last row's outputs."""
    L.require_cuda(ring, win, out)
    tab = ragged.host_table(table, STREAM_RESAMPLE_COLS)
    _stream_ring(ring)
    if win.dim() != 1 or win.dtype != torch.float32 or not win.is_contiguous():
        raise ValueError("win must be a contiguous 1-D float32 tensor")
    if out is None:
        out = torch.empty(max(int((tab[:, 5] + np.maximum(tab[:, 2] - tab[:, 1], 0)).max()), 0), dtype=torch.float32, device=ring.device)
    elif out.dim() != 1 or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous 1-D float32 tensor")
    d_tab = ragged.upload(tab, ring.device)
    L.check(L.lib().sos_stream_resample_f32(L.ptr(ring), ring.shape[0], ring.shape[1], L.ptr(d_tab), tab.ctypes.data, tab.shape[0],
                                            float(ratio), L.ptr(win), win.numel(), int(num_table), L.ptr(out), out.numel(),
                                            L.stream_ptr()), "sos_stream_resample_f32")
    return out


STREAM_BAND_RATIO_COLS, STREAM_BAND_MERGE_COLS = 5, 10                 # int64 per row (csrc/stream_band.hip: SB_*_COLS)


def _stream_band_rings(ring, rring):
    _stream_ring(ring)
    if ring.shape[0] % 3:
        raise ValueError("ring must hold the x, a and b rings of every slot: (3 slots, capacity)")
    if rring is not None and (rring.dim() != 2 or rring.dtype != torch.float64 or not rring.is_contiguous() or
                              rring.shape[0] != ring.shape[0] // 3):
        raise ValueError("rring must be a contiguous float64 (slots, frames) tensor")


def stream_band_ratio(ring, rring, table, hop):
    """r[j] of whole hop frames of streams into their rings of frames in one launch (sos_stream_band_ratio_f64).  ring: (3 slots,
    capacity) f32 GPU tensor, rows slot / slots + slot / 2 slots + slot = x / a / b of a stream as stream_push fills them; rring:
    (slots, frames) f64 GPU tensor, written in place; table: host rows {slot, j_lo, j_hi, m_a, m_b}, a slot at most once."""
    L.require_cuda(ring, rring)
    tab = ragged.host_table(table, STREAM_BAND_RATIO_COLS)
    _stream_band_rings(ring, rring)
    d_tab = ragged.upload(tab, ring.device)
    L.check(L.lib().sos_stream_band_ratio_f64(L.ptr(ring), ring.shape[0] // 3, ring.shape[1], L.ptr(d_tab), tab.ctypes.data, tab.shape[0],
                                              int(hop), L.ptr(rring), rring.shape[1], L.stream_ptr()), "sos_stream_band_ratio_f64")


def stream_band_merge(ring, rring, table, ratio, win, num_table, hop, smooth, out):
    """Outputs of streams with the band above the low rate's half put back, in one launch (sos_stream_band_merge_f32): out[t] =
    fmaf(g[t], x[t] - U(a)[t], U(b)[t]) out of the rings.  table: host rows {slot, t_lo, t_hi, n_x, n_a, n_b, v_b, J, r_hi,
    output offset}, a slot at most once; ratio = native rate / low rate; win, num_table: resampling.filter_on's; smooth: the frames
    of smoothing of g, or None for g = 1 (rring may be None then); out: a contiguous 1-D f32 GPU tensor, written at the rows'
    offsets."""
    L.require_cuda(ring, rring, win, out)
    tab = ragged.host_table(table, STREAM_BAND_MERGE_COLS)
    _stream_band_rings(ring, rring)
    if win.dim() != 1 or win.dtype != torch.float32 or not win.is_contiguous():
        raise ValueError("win must be a contiguous 1-D float32 tensor")
    if out.dim() != 1 or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous 1-D float32 tensor")
    if smooth is not None and rring is None:
        raise ValueError("gains need the ring of frames")
    d_tab = ragged.upload(tab, ring.device)
    L.check(L.lib().sos_stream_band_merge_f32(L.ptr(ring), ring.shape[0] // 3, ring.shape[1], L.ptr(rring),
                                              rring.shape[1] if rring is not None else 0, L.ptr(d_tab), tab.ctypes.data, tab.shape[0],
                                              float(ratio), L.ptr(win), win.numel(), int(num_table), int(hop),
                                              -1 if smooth is None else int(smooth), L.ptr(out), out.numel(), L.stream_ptr()),
            "sos_stream_band_merge_f32")
    return out


def stream_flat(chunks, device):
    """Chunks (1-D f32 GPU tensors or numpy arrays) back to back in one device buffer (host arrays go up in one copy) and where
    each starts: -> (flat or None if all are empty, offsets)."""
    from .engine import upload
    host = [c for c in chunks if not torch.is_tensor(c) and c.shape[0]]
    up = iter(ragged.split(upload(np.concatenate(host), torch.float32, device), [c.shape[0] for c in host]) if host else [])
    parts = [(c.to(device).contiguous() if torch.is_tensor(c) else next(up)) for c in chunks if c.shape[0]]
    flat = (torch.cat(parts) if len(parts) > 1 else parts[0]) if parts else None
    return flat, ragged.offsets([c.shape[0] for c in chunks]).tolist()


def convert_bitstreammask_to_audiomask(ref_audio_signal, frames_to_audiosample_ratio, bitstream):
    """M2/tools.py:340-362 (string bits) / M1/tools.py:770-792 (int bits): same arguments, same
    RuntimeError on an invalid bit, same dtype as `ref_audio_signal`."""
    vals = []
    for bit in bitstream:
        if bit in ('0', 0):
            vals.append(0)
        elif bit in ('1', 1):
            vals.append(1)
        else:
            print('Invalid bit?')
            raise RuntimeError
    if not torch.cuda.is_available():
        raise RuntimeError("sos_amd.tools needs an MI355X: there is no CPU fallback")
    bits = torch.tensor(vals, dtype=torch.uint8, device="cuda").reshape(1, -1)
    n = len(ref_audio_signal)
    mask = bits_to_mask_batch(bits, frames_to_audiosample_ratio, n)
    return mask[0].cpu().numpy().astype(np.asarray(ref_audio_signal).dtype)


def threshold_bits(logits, threshold=0.5):
    """M1/predict.py:117-119: bit = sigmoid(logit) >= threshold (1 = non-silent); returns
    (bits uint8, confidence f32) with the shape of `logits`."""
    L.require_cuda(logits)
    lg = logits.contiguous().float()
    bits = torch.empty(lg.shape, dtype=torch.uint8, device=lg.device)
    conf = torch.empty_like(lg)
    L.check(L.lib().sos_threshold_bits(L.ptr(lg), lg.numel(), float(threshold), L.ptr(bits), L.ptr(conf),
                                       L.stream_ptr()), "sos_threshold_bits")
    return bits, conf


def add_signals_batch(signal, noises, snr, norm=0.5):
    """Batched, on-device `add_signals`: signal f32 (B, n), noises f32 (B, K, n) or (B, n), snr scalar / sequence / tensor
    of B values (dB) -> (mixed (B, n), signal (B, n), noises like the input), GPU tensors."""
    L.require_cuda(signal, noises)
    signal = signal.contiguous().float()
    squeeze = noises.dim() == 2
    nz = (noises[:, None] if squeeze else noises).contiguous().float()
    B, n = signal.shape
    if nz.shape[0] != B or nz.shape[2] != n or not 1 <= nz.shape[1] <= 8:
        raise ValueError("noises must be (B, K <= 8, n) matching signal (B, n)")
    snr_t = torch.as_tensor(snr, dtype=torch.float32).reshape(-1)
    snr_t = (snr_t.expand(B) if snr_t.numel() == 1 else snr_t).contiguous().to(signal.device)
    if snr_t.numel() != B:
        raise ValueError("snr must be a scalar or one value per clip")
    mixed, s_out, n_out = torch.empty_like(signal), torch.empty_like(signal), torch.empty_like(nz)
    L.check(L.lib().sos_add_signals_f32(L.ptr(signal), L.ptr(nz), L.ptr(snr_t), B, nz.shape[1], n, float(norm or 0.0),
                                        L.ptr(mixed), L.ptr(s_out), L.ptr(n_out), L.stream_ptr()), "sos_add_signals_f32")
    return mixed, s_out, (n_out[:, 0] if squeeze else n_out)


def add_signals(signal, noises, snr, norm=0.5):
    """M2/tools.py:217-276 with its arguments and its return triple (mixed, signal, [noises]): numpy in, numpy out, the
    arithmetic in sos_add_signals_f32."""
    if not torch.cuda.is_available():
        raise RuntimeError("sos_amd.tools needs an MI355X: there is no CPU fallback")
    single = not isinstance(noises, (list, tuple))
    stack = np.stack([np.asarray(x, dtype=np.float32) for x in ([noises] if single else noises)])
    sig = torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float32)).cuda()[None]
    m, s, nz = add_signals_batch(sig, torch.from_numpy(stack).cuda()[None], float(snr), norm)
    dt = np.asarray(signal).dtype if np.issubdtype(np.asarray(signal).dtype, np.floating) else np.float32
    return m[0].cpu().numpy().astype(dt), s[0].cpu().numpy().astype(dt), [x.cpu().numpy().astype(dt) for x in nz[0]]


_MIX_OUT = 6                        # f64 per clip of sos_ragged_mix_f32: Es, Ez, gain, peak, inv, status


def _mix_1d(x, name, i, dtype_ok, what):
    """The length of entry i of a list of 1-D arrays / tensors, or ValueError."""
    dt, shape = (x.dtype, tuple(x.shape)) if torch.is_tensor(x) else (np.asarray(x).dtype, np.shape(x))
    if len(shape) != 1 or not dtype_ok(dt):
        raise ValueError(f"{name}[{i}]: a 1-D {what} array or tensor, got shape {shape} of {dt}")
    return int(shape[0])


def _mix_float(dt):
    return dt.is_floating_point if isinstance(dt, torch.dtype) else np.issubdtype(dt, np.floating)


def _mix_plan(signals, noises, snr, noise_index, starts, counts, bits, ratios, norm):
    """The host side of add_signals_ragged, checked before anything goes up: per-clip lengths, crops {noise, start, valid
    samples}, parameters {snr, ratio or 0} and frame counts."""
    B = len(signals)
    lens = [_mix_1d(s, "signals", i, _mix_float, "floating-point") for i, s in enumerate(signals)]
    for i, n in enumerate(lens):
        if n < 1:
            raise ValueError(f"signals[{i}] is empty")
    nlens = [_mix_1d(z, "noises", i, _mix_float, "floating-point") for i, z in enumerate(noises)]
    if B and not nlens:
        raise ValueError("no noise recordings")
    if noise_index is None:
        if len(noises) != B:
            raise ValueError(f"noise_index=None pairs clip i with noise i: {B} clips, {len(noises)} noises")
        noise_index = range(B)
    index = np.asarray(list(noise_index), dtype=np.int64).reshape(-1)
    if len(index) != B:
        raise ValueError(f"noise_index: one entry per clip ({B}), got {len(index)}")
    if B and (index.min() < 0 or index.max() >= len(noises)):
        raise ValueError(f"noise_index names a recording outside the {len(noises)} noises")
    start = ragged.per_clip(starts, B, "starts")
    count = ragged.per_clip(lens if counts is None else counts, B, "counts")
    if np.any(start < 0) or np.any(count < 0) or np.any(start != np.floor(start)) or np.any(count != np.floor(count)):
        raise ValueError("starts and counts are non-negative whole numbers of samples")
    par = np.zeros((B, 2), dtype=np.float64)
    par[:, 0] = ragged.per_clip(snr, B, "snr")
    if not np.all(np.isfinite(par[:, 0])):
        raise ValueError("snr must be finite")
    if not np.isfinite(float(norm or 0.0)):
        raise ValueError("norm must be finite")
    nb = [0] * B
    if bits is not None:
        if len(bits) != B:
            raise ValueError(f"bits: one entry (or None) per clip ({B}), got {len(bits)}")
        if isinstance(ratios, (list, tuple)):                            # (a None entry goes with a None entry of bits)
            ratios = [0.0 if r is None else r for r in ratios]
        rat = ragged.per_clip(0.0 if ratios is None else ratios, B, "ratios")
        for i, b in enumerate(bits):
            if b is None:
                continue
            nb[i] = _mix_1d(b, "bits", i, lambda dt: dt in (torch.uint8, np.dtype(np.uint8)), "uint8")
            if nb[i] < 1:
                raise ValueError(f"bits[{i}] is empty")
            if not (rat[i] > 1.0 and np.isfinite(rat[i])):
                raise ValueError(f"ratios[{i}] = {rat[i]!r}: a clip with frame decisions needs more than one sample per frame")
            par[i, 1] = rat[i]
    crop = np.zeros((B, 3), dtype=np.int64)
    crop[:, 0], crop[:, 1] = index, start
    avail = np.asarray(nlens, dtype=np.int64)[index] - crop[:, 1] if B else crop[:, 1]
    crop[:, 2] = np.clip(np.minimum(np.minimum(count, lens), avail), 0, None)
    crop[crop[:, 2] == 0, 1] = 0                                         # an empty crop starts anywhere: keep it inside
    return lens, nlens, crop, par, nb


_MixStaged = namedtuple("_MixStaged", "flat lens tab d_tab d_noise noise_total ntab d_ntab d_bits par d_par norm ws mixed clean noise out")


def _mix_stage(signals, d_noise, noise_total, ntab, par, bits, nb, norm):
    """One launch sequence's worth of clips (at most ragged.MAX_CLIPS) on the device: the concatenated samples, the tables and
    parameters (host and device), the frame decisions, the workspace and the result buffers."""
    flat, lens = ragged.concat(signals)
    dev, B = flat.device, len(lens)
    tab = ragged.clip_table(lens, nb)
    d_bits = None
    if any(nb):
        some = [b for b in bits if b is not None]
        if any(torch.is_tensor(b) for b in some):
            d_bits = torch.cat([b.to(dev) if torch.is_tensor(b) else torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in some])
        else:
            d_bits = torch.from_numpy(np.concatenate([np.asarray(b, dtype=np.uint8) for b in some])).to(dev)
    nbytes = L.lib().sos_ragged_mix_workspace_bytes(tab.ctypes.data, B)
    if nbytes < 0:
        L.check(-22, "sos_ragged_mix_workspace_bytes")
    total = int(tab[:, 1].sum())
    mixed, clean, noise = (torch.empty(total, dtype=torch.float32, device=dev) for _ in range(3))
    return _MixStaged(flat, lens, tab, ragged.upload(tab, dev), d_noise, noise_total, ntab, ragged.upload(ntab, dev), d_bits, par,
                      ragged.upload(par, dev), float(norm or 0.0), torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev),
                      mixed, clean, noise, torch.empty((B, _MIX_OUT), dtype=torch.float64, device=dev))


def _mix_launch(st):
    """Enqueue sos_ragged_mix_f32 on staged clips; no wait."""
    L.check(L.lib().sos_ragged_mix_f32(L.ptr(st.flat), L.ptr(st.d_tab), st.tab.ctypes.data, len(st.tab), L.ptr(st.d_noise),
                                       st.noise_total, L.ptr(st.d_ntab), st.ntab.ctypes.data, L.ptr(st.d_bits), L.ptr(st.d_par),
                                       st.par.ctypes.data, st.norm, L.ptr(st.ws), st.ws.numel(), L.ptr(st.mixed), L.ptr(st.clean),
                                       L.ptr(st.noise), L.ptr(st.out), L.stream_ptr()), "sos_ragged_mix_f32")
    return st


def add_signals_ragged(signals, noises, snr, noise_index=None, starts=0, counts=None, bits=None, ratios=None, norm=0.5,
                       return_detail=False):
    """`add_signals` with one noise (M2/tools.py:217-276) for clips of any lengths in one launch sequence
    (sos_ragged_mix_f32; float64 restatement: tests/mix_reference.py).  signals: a list of 1-D clips, numpy arrays or GPU
    tensors; noises: a list of 1-D noise recordings, uploaded once per call; noise_index[i] names the recording of clip i
    (default i: as many noises as clips).  Clip i is mixed with noise[start : start + count] (starts / counts: a scalar or one
    value per clip; counts defaults to the clip's length), clipped to the recording and to the clip's length and zero-filled
    beyond -- the crop of handoff.add_noise_to_audio.  snr: dB, a scalar or one value per clip.  bits / ratios: per-clip uint8
    frame decisions (1 = non-silent) and samples per frame as pipeline.denoise_ragged(bits=) takes them; the clip is silenced
    on its silent intervals (bits_to_mask_batch's mask) before mixing; a None entry leaves the clip as it is.  norm: the peak
    of the mix (None / 0: no normalisation).
    -> (mixed, clean, noise): three lists of 1-D f32 GPU tensors in input order, views into three flat buffers (per
    ragged.MAX_CLIPS clips), so ragged.download brings a whole batch down in one copy.  return_detail=True adds a list of
    dict(signal_energy, noise_energy, gain, peak, inv).  A clip's results are the same bits alone, in any batch and in any
    order.  One wait per call (the status rows).  Argument errors are ValueErrors raised before anything is uploaded."""
    signals, noises = list(signals), list(noises)
    bits = None if bits is None else list(bits)
    lens, nlens, crop, par, nb = _mix_plan(signals, noises, snr, noise_index, starts, counts, bits, ratios, norm)
    B = len(signals)
    mixed, clean, noise, detail = [], [], [], []
    if not B:
        return (mixed, clean, noise, detail) if return_detail else (mixed, clean, noise)
    d_noise, _ = ragged.concat(noises)
    ntab = np.ascontiguousarray(np.stack([ragged.offsets(nlens)[crop[:, 0]] + crop[:, 1], crop[:, 2]], axis=1))
    done = []
    for c0 in range(0, B, ragged.MAX_CLIPS):
        c1 = min(B, c0 + ragged.MAX_CLIPS)
        done.append(_mix_launch(_mix_stage(signals[c0:c1], d_noise, int(sum(nlens)), np.ascontiguousarray(ntab[c0:c1]),
                                           np.ascontiguousarray(par[c0:c1]), None if bits is None else bits[c0:c1], nb[c0:c1],
                                           norm)))
    rows = torch.cat([st.out for st in done]).cpu().numpy()              # the one wait of the call
    bad = np.flatnonzero(rows[:, 5] < 0)
    if len(bad):
        raise RuntimeError(f"sos_ragged_mix_f32: clip {int(bad[0])}: the device tables disagree with the host's")
    for st in done:
        mixed += ragged.split(st.mixed, st.lens)
        clean += ragged.split(st.clean, st.lens)
        noise += ragged.split(st.noise, st.lens)
    if not return_detail:
        return mixed, clean, noise
    detail = [dict(signal_energy=float(r[0]), noise_energy=float(r[1]), gain=float(r[2]), peak=float(r[3]), inv=float(r[4]))
              for r in rows]
    return mixed, clean, noise, detail


def trim_unknown_frames(bits):
    """M1/tools.py:270-274,306-311 (`truncate`): the first two runs of '2' (unlabelled frames) bound the labelled part
    of a bit-stream; a stream without two such runs is used whole.  Returns (first, end) frame indices.  One helper
    for the file data loader and the on-disk hand-off."""
    from itertools import groupby
    runs = [len(list(g)) for k, g in groupby(bits) if k == '2']
    if len(runs) >= 2:
        return runs[0], len(bits) - runs[1]
    return 0, len(bits)
