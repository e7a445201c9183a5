"""Channel planes (csrc/pcm_io.hip, csrc/loudness.hip, csrc/limiter.hip): the samples of WAVE files, as wave_file.py reads them,
decoded into one f32 plane per channel on the GPU, and planes encoded back into the data bytes of a file -- the linear formats and
G.711 -- with the gain that brings a file to a target loudness, and the look-ahead limiter, in between.  No CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ragged
from .resampling import resample_batch_device
from .wave_file import DECODE, ENCODINGS, G711, read_wave_info


def pcm_to_mono_device(pcm, fmt):
    """pcm: (n_frames, channels) device tensor of int16 / int32 / float32 / uint8, or of uint8 G.711 codes with fmt 'alaw' /
    'ulaw' -> mono f32 (n_frames,)."""
    L.require_cuda(pcm)
    pcm = pcm.contiguous()
    n, ch = pcm.shape
    out = torch.empty(n, dtype=torch.float32, device=pcm.device)
    family, code = DECODE[fmt]
    name = "sos_g711_to_mono_f32" if family == "g711" else "sos_pcm_to_mono_f32"
    L.check(getattr(L.lib(), name)(L.ptr(pcm), code, ch, n, L.ptr(out), L.stream_ptr()), name)
    return out


def check_planes(who, planes):
    """`planes` as a list of one (1 .. 64 channels, n) float32 tensor per file, or `who`'s ValueError."""
    planes = list(planes)
    for i, p in enumerate(planes):
        if not torch.is_tensor(p) or p.dim() != 2 or p.dtype != torch.float32 or not 1 <= p.shape[0] <= 64:
            raise ValueError("%s: file %d must be a (1 .. 64 channels, n) float32 tensor" % (who, i))
    return planes


def plane_frames(who, planes, frames):
    """The samples per channel that count, per file: `frames` (default: each plane's n) as a list of ints, or `who`'s ValueError."""
    frames = [int(p.shape[1]) for p in planes] if frames is None else [int(f) for f in frames]
    if len(frames) != len(planes) or min(frames, default=0) < 0:
        raise ValueError("%s: frames holds one non-negative count per file" % who)
    return frames


def planes_flat(planes):
    """The planes of a non-empty list of files as one 1-D buffer (never a null pointer: one zero where no file has a sample) and
    the per-file int64 arrays (first sample in it, channels, samples per channel)."""
    chans = np.asarray([p.shape[0] for p in planes], dtype=np.int64)
    avail = np.asarray([p.shape[1] for p in planes], dtype=np.int64)
    flat = ragged.back_to_back(planes) if int((chans * avail).sum()) else torch.zeros(1, dtype=torch.float32, device=planes[0].device)
    return flat, ragged.offsets(chans * avail), chans, avail


def planes_of(channels):
    """The equally long 1-D f32 GPU tensors of one file's channels as one (channels, n) tensor (a view if they lie back to back)."""
    return ragged.back_to_back(list(channels)).view(len(channels), -1)


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
    for i, (a, k) in enumerate(zip(arrs, kinds)):
        if k not in DECODE:
            raise ValueError("decode_planes_batch_device: file %d has the unsupported sample format %r" % (i, k))
        if a.ndim != 2 or not 1 <= a.shape[1] <= 64:
            raise ValueError("decode_planes_batch_device: file %d must be (frames, 1 .. 64 channels), got shape %s" % (i, a.shape))
    by_kind = ragged.group_by(kinds, lambda i, k: not arrs[i].shape[0])
    if not torch.cuda.is_available():
        raise RuntimeError("sos_amd.audio_io needs an MI355X: there is no CPU fallback")
    sizes = np.asarray([a.size for a in arrs], dtype=np.int64)
    order = [i for idx in by_kind.values() for i in idx]
    out = torch.empty(int(sizes.sum()), dtype=torch.float32, device=device)
    where = dict(zip(order, ragged.offsets(sizes[order]).tolist()))
    h = L.lib()
    for k, idx in by_kind.items():
        family, code = DECODE[k]
        name = "sos_g711_planes_batch_f32" if family == "g711" else "sos_pcm_planes_batch_f32"
        pcm = torch.from_numpy(np.concatenate([arrs[i].reshape(-1) for i in idx])).to(device)
        off = ragged.offsets(sizes[idx])
        for c0, c1 in ragged.chunks(len(idx)):
            sel = idx[c0:c1]
            o0 = where[sel[0]]
            tab, tab_dev = ragged.table([[off[c0 + j] - off[c0], arrs[i].shape[0], arrs[i].shape[1], where[i] - o0]
                                         for j, i in enumerate(sel)], device)
            L.check(getattr(h, name)(L.ptr(pcm[int(off[c0]):]), code, L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), len(sel),
                                     L.ptr(out[o0:]), L.stream_ptr()), name)
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

    def at_sr(r, idx):
        outs = iter(resample_batch_device([ys[i][c] for i in idx for c in range(ys[i].shape[0])], r, sr, res_type))
        return [planes_of([next(outs) for _ in range(ys[i].shape[0])]) for i in idx]

    return ragged.per_group(ys, rates, at_sr, lambda i, r: r == sr or not ys[i].shape[1]), [sr] * len(paths), infos


DITHER = {"tpdf": 1, "highpass": 2}        # SOS_DITHER_* of include/sos_hip.h
DITHER_FORMATS = ("u8", "s16", "s24")      # s32 holds more bits than a float32, f32 is a copy, G.711 drops the low bits
FRAME_LIMIT = 1 << 62                       # frame0 + frames may not pass it


def _dither_columns(who, fmt, dither, seed, keys, frame0, frames):
    """The checked dither arguments of encode_batch_device: int64 arrays (file keys, first absolute frames), or its ValueError."""
    if dither not in DITHER:
        raise ValueError("%s: unknown dither %r (one of %s, or None)" % (who, dither, ", ".join(sorted(DITHER))))
    if fmt not in DITHER_FORMATS:
        raise ValueError("%s: sample format %r takes no dither (%s do)" % (who, fmt, ", ".join(DITHER_FORMATS)))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError("%s: the dither seed is an integer in 0 .. 2^64 - 1, got %r" % (who, seed))
    cols = []
    for name, given, default, top in (("keys", keys, range(len(frames)), lambda f: (1 << 32) - 1),
                                      ("frame0", frame0, [0] * len(frames), lambda f: FRAME_LIMIT - int(frames[f]))):
        vals = list(default if given is None else given)
        if len(vals) != len(frames):
            raise ValueError("%s: %s holds one integer per file (%d files, %d given)" % (who, name, len(frames), len(vals)))
        for f, v in enumerate(vals):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= top(f):
                raise ValueError("%s: %s[%d] = %r is outside 0 .. %d" % (who, name, f, v, top(f)))
        cols.append(np.asarray([int(v) for v in vals], dtype=np.int64))
    return cols


def encode_batch_device(planes, fmt, frames=None, dither=None, seed=0, keys=None, frame0=None):
    """planes: one (channels, n) f32 GPU tensor per file; fmt: 's16', 's24' (packed, 3 bytes little-endian), 's32', 'u8' or
    'f32'; frames: samples per channel to write per file (default: n).  -> (data, offsets, clipped): one uint8 GPU tensor with
    the files' interleaved [frames][channels] data back to back, the host int64 byte offsets (files + 1 entries) and an int64
    GPU tensor of per-file counts, from ONE sos_pcm_encode_batch launch (per 65535 files).  Per sample: the plane's value below
    n and 0 from there to `frames` (crop / zero-fill happen in the kernel); f32 copies the bits; otherwise q = rint(x * S) half
    to even in double with S = 2^(bits-1), NaN -> 0, saturated to [-S, S - 1]; u8 stores q + 128.  clipped[f] counts the samples
    that were NaN or changed by saturation (+-inf included).  Float64 restatement: tests/pcm_reference.py.
    dither=None (the default) is plain rounding: the quantisation error is correlated with the signal, as with soundfile's and
    scipy's integer writers, and a component below half an LSB is gated to zero.  dither='tpdf' / 'highpass' ('u8', 's16', 's24'
    only; ONE sos_pcm_encode_dither_batch launch) adds d LSB before the one rounding, q = rint(x * S + d): 'tpdf' is triangular
    on (-1, 1), white; 'highpass' the difference of two successive uniform draws, the same marginal with its power moved towards
    fs / 2 (it shapes the dither only: the quantisation error is not fed back).  Either makes the mean and the variance of the
    total error free of the signal, at a noise floor of 1/4 LSB^2 in place of 1/12.  d is a pure function of (seed, keys[f],
    channel, frame0[f] + frame) -- Philox4x32-10 evaluated inside the kernel (csrc/dither_core.h; numpy restatement:
    tests/dither_reference.py) -- so a file's bytes depend neither on the other files of the call nor on how a signal was cut
    into calls: encode the packets of a live leg with the same key and frame0 advanced by each packet's length and they
    concatenate to the encode of the whole.  seed: 0 .. 2^64 - 1; keys: one integer 0 .. 2^32 - 1 per file (default: the
    file's position in `planes`); frame0: one integer 0 .. 2^62 - frames per file (default 0).  Every written sample is dithered,
    the zero-fill included, and `clipped` counts after the dither.  ValueError before any launch: an unknown dither, another
    format, a seed, key or frame0 out of range, keys / frame0 not one per file.
    'alaw' / 'ulaw' (G.711, one code byte per sample, ONE sos_g711_encode_batch launch): the 's16' value q, counted as 's16'
    counts it, through the reference compressor (include/sos_hip.h; it drops the low bits of q, as audioop, libsndfile and sox
    do); the zero-fill is the code of silence, 0xD5 / 0xFF.  Restatement: tests/g711_reference.py."""
    who = "encode_batch_device"
    if fmt not in ENCODINGS and fmt not in G711:
        raise ValueError("encode_batch_device: unsupported sample format %r (one of %s)"
                         % (fmt, ", ".join(sorted(ENCODINGS) + sorted(G711))))
    code, width = (G711[fmt] if fmt in G711 else ENCODINGS[fmt])[:2]
    name = "sos_g711_encode_batch" if fmt in G711 else "sos_pcm_encode_batch" if dither is None else "sos_pcm_encode_dither_batch"
    planes = check_planes(who, planes)
    frames = np.asarray(plane_frames(who, planes, frames), dtype=np.int64)
    extra = () if dither is None else tuple(_dither_columns(who, fmt, dither, seed, keys, frame0, frames))
    how = () if dither is None else (DITHER[dither], C.c_uint64(int(seed)))
    L.require_cuda(*planes)
    elems = np.asarray([p.shape[0] for p in planes], dtype=np.int64) * frames
    offsets = np.concatenate([ragged.offsets(elems), [elems.sum()]]).astype(np.int64) * width
    if not planes:
        return torch.zeros(0, dtype=torch.uint8, device="cuda"), offsets, torch.zeros(0, dtype=torch.int64, device="cuda")
    device = planes[0].device
    flat, src, chans, avail = planes_flat(planes)
    data = torch.empty(max(int(offsets[-1]), 1), dtype=torch.uint8, device=device)
    clipped = torch.empty(len(planes), dtype=torch.int64, device=device)
    h = L.lib()
    for c0, c1 in ragged.chunks(len(planes)):
        e0 = int(offsets[c0]) // width
        tab, tab_dev = ragged.table(np.stack([src[c0:c1] - src[c0], avail[c0:c1], chans[c0:c1], frames[c0:c1],
                                              offsets[c0:c1] // width - e0] + [col[c0:c1] for col in extra], axis=1), device)
        L.check(getattr(h, name)(L.ptr(flat[int(src[c0]):]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0, code, *how,
                                 L.ptr(data[e0 * width:]), L.ptr(clipped[c0:]), L.stream_ptr()), name)
    return data[:int(offsets[-1])], offsets, clipped


def planes_together(planes):
    """The (channels, n) f32 GPU tensors of a group of files as views into ONE buffer, files back to back: the tensors
    themselves where they already lie so, views into one copy otherwise."""
    planes = list(planes)
    if not planes:
        return planes
    flat = ragged.back_to_back(planes)
    if flat.untyped_storage().data_ptr() == planes[0].untyped_storage().data_ptr():
        return planes
    return [v.view(p.shape) for v, p in zip(ragged.split(flat, [p.numel() for p in planes]), planes)]


def _level_args(who, planes, stats, target, peak_ceiling_db, frames):
    """The checked arguments loudness_gain_batch_device and limit_batch_device share: (planes, rows f64 [files][4], targets f64
    [files] on the device or None without a file, frames), or `who`'s ValueError."""
    planes = check_planes(who, planes)
    rows = stats["rows"] if isinstance(stats, dict) else stats
    if not torch.is_tensor(rows) or rows.dtype != torch.float64 or tuple(rows.shape) != (len(planes), 4):
        raise ValueError("%s: stats holds one float64 row of 4 per file (metrics.loudness_batch)" % who)
    if torch.is_tensor(target):
        if target.dtype != torch.float64 or tuple(target.shape) != (len(planes),):
            raise ValueError("%s: a target tensor holds one float64 per file" % who)
    elif not np.isfinite(float(target)):
        raise ValueError("%s: the target is a finite number of LUFS, got %r" % (who, target))
    if not float(peak_ceiling_db) <= 0.0:
        raise ValueError("%s: the ceiling is at most 0 dBFS, got %r" % (who, peak_ceiling_db))
    frames = plane_frames(who, planes, frames)
    L.require_cuda(rows, *planes)
    if not planes:
        return planes, rows, None, frames
    if torch.is_tensor(target):
        L.require_cuda(target)
        targets = target.contiguous()
    else:
        targets = torch.full((len(planes),), float(target), dtype=torch.float64, device=planes[0].device)
    return planes, rows.contiguous(), targets, frames


def loudness_gain_batch_device(planes, stats, target, peak_ceiling_db=-1.0, frames=None):
    """Brings every file of a group to a target loudness, IN PLACE and in one sos_loudness_gain_batch_f32 launch (per 65535
    files), without a wait.  planes: one (channels, n) f32 GPU tensor per file; stats: what metrics.loudness_batch returned for
    them (its dict, or the f64 [files][4] rows {L, peak, ..}); target: LUFS, one float for all files or an f64 GPU tensor of one
    per file (the 'source' mode hands over the loudness it measured, still on the device); peak_ceiling_db: dBFS (<= 0) the
    SAMPLE peak of the scaled file may reach; frames: samples per channel to scale per file (default n; what lies past them
    keeps its value).  Per file, in float64, g = min(10^((target - L) / 20), 10^(ceiling / 20) / peak), stored as float32; g = 1
    where L is -inf (no block passed the gates), the peak is 0 or the target is not finite; out = x * g, one float32 multiply.
    -> (gains f32 [files], limited bool [files]: the ceiling bound the gain), on the device.  Float64 restatement:
    tests/loudness_reference.py.
    A TRUE-PEAK ceiling (dBTP, what EBU R128 delivery asks for): hand over metrics.loudness_batch(.., true_peak=True)["rows_true"],
    the rows with the true peak in column 1.  g = min(10^((target - L) / 20), 10^(ceiling / 20) / true peak); the interpolation
    is linear, so the scaled file's true peak is g * the measured one up to float32 rounding, and stays at or below the ceiling."""
    who = "loudness_gain_batch_device"
    planes, rows, targets, frames = _level_args(who, planes, stats, target, peak_ceiling_db, frames)
    if not planes:
        return torch.zeros(0, dtype=torch.float32, device="cuda"), torch.zeros(0, dtype=torch.bool, device="cuda")
    device = planes[0].device
    together = planes_together(planes) if sum(p.numel() for p in planes) else planes
    flat, src, chans, avail = planes_flat(together)
    gains = torch.empty(len(planes), dtype=torch.float32, device=device)
    limited = torch.empty(len(planes), dtype=torch.int32, device=device)
    h = L.lib()
    for c0, c1 in ragged.chunks(len(planes)):
        tab = np.zeros((c1 - c0, 8), dtype=np.int64)
        tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3] = src[c0:c1] - src[c0], avail[c0:c1], chans[c0:c1], frames[c0:c1]
        tab_dev = ragged.upload(tab, device)
        L.check(h.sos_loudness_gain_batch_f32(L.ptr(flat[int(src[c0]):]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0,
                                              L.ptr(rows[c0:]), L.ptr(targets[c0:]), float(peak_ceiling_db), L.ptr(gains[c0:]),
                                              L.ptr(limited[c0:]), L.stream_ptr()), "sos_loudness_gain_batch_f32")
    for p, t in zip(planes, together):
        if t is not p:                                  # the planes lay apart: the launch scaled their copy
            p.copy_(t)
    return gains, limited.bool()


LIMITER_TILE = 4096                 # samples of time per workgroup of sos_limiter_batch_f32: SOS_LIMITER_TILE of include/sos_hip.h
LIMITER_MAX_LOOKAHEAD = 1024        # samples


def limiter_lookahead(who, rates, lookahead_ms, nfiles):
    """H = round(lookahead_ms * rate / 1000) per file as a list of ints, or `who`'s ValueError: a look-ahead that is not finite
    and positive, rates that are not one per file, a file whose rate puts H outside 1 .. 1024 samples."""
    ok = not isinstance(lookahead_ms, (bool, str)) and np.ndim(lookahead_ms) == 0 and np.isfinite(float(lookahead_ms))
    if not ok or float(lookahead_ms) <= 0.0:
        raise ValueError("%s: lookahead_ms is a finite number of milliseconds above 0, got %r" % (who, lookahead_ms))
    if rates is None:
        raise ValueError("%s: rates= is needed (one sample rate per file, or one for all)" % who)
    rates = [rates] * nfiles if np.ndim(rates) == 0 else list(rates)
    if len(rates) != nfiles:
        raise ValueError("%s: one rate per file (%d files, %d rates)" % (who, nfiles, len(rates)))
    out = []
    for i, r in enumerate(rates):
        if isinstance(r, bool) or not np.isfinite(float(r)) or float(r) <= 0.0:
            raise ValueError("%s: file %d has the rate %r (a positive number of Hz)" % (who, i, r))
        out.append(int(round(float(lookahead_ms) * float(r) / 1000.0)))
        if not 1 <= out[-1] <= LIMITER_MAX_LOOKAHEAD:
            raise ValueError("%s: file %d: %r ms at %r Hz is a look-ahead of %d samples (1 .. %d)"
                             % (who, i, lookahead_ms, r, out[-1], LIMITER_MAX_LOOKAHEAD))
    return out


def limit_batch_device(planes, stats, target, peak_ceiling_db=-1.0, rates=None, lookahead_ms=5.0, frames=None, true_peak=False):
    """The look-ahead limiter: every file of a group at the gain that brings it to its target loudness, with its peaks held at
    the ceiling by a gain that dips around them only, where loudness_gain_batch_device lowers the whole file.  OUT OF PLACE, one
    sos_limiter_batch_f32 launch sequence (per 65535 files), without a wait.  planes, stats, target, peak_ceiling_db and frames
    as loudness_gain_batch_device takes them (the ceiling bounds the SAMPLE peak; true_peak=True: the true peak, by the
    interpolator of metrics.true_peak_batch); rates: the sample rate per file, or one for all; lookahead_ms: H = round(lookahead_ms
    * rate / 1000) samples per file, 1 .. 1024.
    Per file, ONE gain curve for all channels (a stereo image does not shift), samples past min(frames, n) reading 0:
    s = float32(10^((target - L) / 20)), 1 where L or the target is not finite; p[t] = the largest |x[t]| of any channel (true_peak:
    and of the six interpolated points next to t); r[t] = min(1, C / (s p[t])), at least 2^-10; mn[t] = min r[t - H .. t + H]; g[t] =
    mean mn[t - H .. t + H], in float64 and exact; out = x * (g * s).  g[t] <= r[t], so the SAMPLE peak of the output is at most
    the ceiling (to 3 ulp); g ramps linearly over 2 H samples on either side of a peak; where no peak is within 2 H samples g is 1
    and the sample is bit for bit what loudness_gain_batch_device writes without a binding ceiling.  Under true_peak the curve is
    built from the true-peak envelope, but a gain that varies between two samples leaves an overshoot of the order H^-1: trim with
    loudness_gain_batch_device on a measurement of the output where the ceiling has to hold strictly (recordings.py does).
    Float64 / numpy restatement: tests/limiter_reference.py.
    -> (limited: one (channels, n) f32 tensor per file, views into ONE new buffer, the samples past `frames` copied; rows: f64
    [files][4] = {s, the least g, the samples with g < 1, 0}), on the device.  ValueError before any launch:
    loudness_gain_batch_device's, a lookahead_ms that is not finite and positive, rates missing or not one per file, a file whose
    rate puts H outside 1 .. 1024."""
    who = "limit_batch_device"
    planes, rows, targets, frames = _level_args(who, planes, stats, target, peak_ceiling_db, frames)
    if not np.isfinite(float(peak_ceiling_db)):
        raise ValueError("%s: the ceiling is a finite level of at most 0 dBFS, got %r" % (who, peak_ceiling_db))
    hs = limiter_lookahead(who, rates, lookahead_ms, len(planes))
    if not planes:
        return [], torch.zeros((0, 4), dtype=torch.float64, device="cuda")
    from .metrics import true_peak_filter                            # metrics imports this module
    device = planes[0].device
    together = planes_together(planes) if sum(p.numel() for p in planes) else planes
    flat, src, chans, avail = planes_flat(together)
    out = torch.empty_like(flat)
    coef = torch.from_numpy(true_peak_filter()).to(device) if true_peak else None
    result = torch.empty((len(planes), 4), dtype=torch.float64, device=device)
    h = L.lib()
    for c0, c1 in ragged.chunks(len(planes)):
        tab = np.zeros((c1 - c0, 8), dtype=np.int64)
        tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3], tab[:, 4] = src[c0:c1] - src[c0], avail[c0:c1], chans[c0:c1], frames[c0:c1], hs[c0:c1]
        tab_dev = ragged.upload(tab, device)
        L.check(h.sos_limiter_batch_f32(L.ptr(flat[int(src[c0]):]), L.ptr(out[int(src[c0]):]), L.ptr(tab_dev),
                                        tab.ctypes.data_as(C.c_void_p), c1 - c0, L.ptr(rows[c0:]), L.ptr(targets[c0:]),
                                        float(peak_ceiling_db), int(bool(true_peak)), L.ptr(coef) if true_peak else None,
                                        L.ptr(result[c0:]), L.stream_ptr()), "sos_limiter_batch_f32")
    limited = [out[int(o):int(o) + p.numel()].view(p.shape) if p.numel() else torch.zeros_like(p) for o, p in zip(src, planes)]
    return limited, result


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


def pcm_encode_device(x, fmt, dither=None, seed=0, key=0, frame0=0):
    """g711_encode_device's sibling for linear PCM: one packet of a live leg, x 1-D f32 GPU tensor -> (1-D uint8 GPU tensor of
    the packet's bytes in `fmt`, clipped: int64 GPU tensor of one count), encode_batch_device([x[None]], fmt, dither=, seed=,
    keys=[key], frame0=[frame0]).  Without dither the rule has no state; with it the state is the caller's count of frames: give
    every packet of a leg the same seed and key and advance frame0 by the packet's length, and the packets concatenate to the
    encode of the whole signal."""
    if fmt not in ENCODINGS:
        raise ValueError("pcm_encode_device: unsupported sample format %r (one of %s)" % (fmt, ", ".join(sorted(ENCODINGS))))
    if not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.float32:
        raise ValueError("pcm_encode_device expects a 1-D float32 tensor")
    if dither is None:
        data, _, clipped = encode_batch_device([x.view(1, -1)], fmt)
    else:
        data, _, clipped = encode_batch_device([x.view(1, -1)], fmt, dither=dither, seed=seed, keys=[key], frame0=[frame0])
    return data, clipped
