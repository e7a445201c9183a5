"""The Kaiser-windowed sinc table (resampy 0.2.2 `kaiser_best`, librosa's default) and what runs it over whole signals on the
GPU: resample_device / resample_batch_device (csrc/wave_io.hip) and the band above the lower rate's half put back,
band_gains_batch_device / resample_merge_batch_device (csrc/band_merge.hip).  The same table under audio that is still arriving:
stream_resampling.py.  No CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ragged
from . import transform

# resampy 0.2.2 `kaiser_best`: 64 zero crossings, 2**9 table points per crossing, Kaiser beta, roll-off
KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)

_filters = {}


def sinc_window(num_zeros, precision, beta, rolloff):
    """Half of a Kaiser-windowed sinc low-pass, `2**precision` points per zero crossing (resampy
    filters.sinc_window with window=kaiser(beta)).  Returns (half_window f64, num_table)."""
    num_table = 2 ** precision
    n = num_table * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_table


def filter_on(device, ratio, res_type):
    """The filter's half window on `device`, scaled by min(1, ratio), and its points per zero crossing; kept per (device, ratio)."""
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
    win, num_table = filter_on(x.device, ratio, res_type)
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
    win, num_table = filter_on(clips[0].device, ratio, res_type)
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
    for c0, c1 in ragged.chunks(len(clips)):
        i0, o0 = int(in_off[c0]), int(out_off[c0])
        tiles = -(-n_out[c0:c1] // L.RESAMPLE_CHUNK)
        tab, tab_dev = ragged.table([in_off[c0:c1] - i0, n_in[c0:c1], out_off[c0:c1] - o0, n_out[c0:c1], n_valid[c0:c1],
                                     ragged.offsets(tiles)], x.device)
        L.check(h.sos_resample_batch_f32(L.ptr(x[i0:]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0, ratio, L.ptr(win),
                                         win.numel(), num_table, L.ptr(out[o0:]), L.stream_ptr()), "sos_resample_batch_f32")
    return ragged.split(out, n_out)


# ------------------------------------------------------------------------------------ the band above SR / 2 (csrc/band_merge.hip)
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
    a, b = ragged.flat_f32(lows_in, device), ragged.flat_f32(lows_out, device)
    gains = torch.empty(int(J.sum()), dtype=torch.float32, device=device)
    h = L.lib()
    for c0, c1 in ragged.chunks(len(lows_in)):
        a0, b0, g0 = int(a_off[c0]), int(b_off[c0]), int(g_off[c0])
        tab, tab_dev = ragged.table([a_off[c0:c1] - a0, m[c0:c1], b_off[c0:c1] - b0, mp[c0:c1], g_off[c0:c1] - g0, J[c0:c1]], device)
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
    win, num_table = filter_on(device, ratio, res_type)
    n = np.asarray([x.numel() for x in natives], dtype=np.int64)
    m = np.asarray([a.numel() for a in lows_in], dtype=np.int64)
    mp = np.asarray([b.numel() for b in lows_out], dtype=np.int64)
    J = -(-m // hop)
    x_off, a_off, b_off, g_off = ragged.offsets(n), ragged.offsets(m), ragged.offsets(mp), ragged.offsets(J)
    x, a, b = ragged.back_to_back(natives), ragged.back_to_back(lows_in), ragged.back_to_back(lows_out)
    s = ragged.back_to_back(gains) if gains is not None else None
    out = torch.empty(int(n.sum()), dtype=torch.float32, device=device)
    h = L.lib()
    for c0, c1 in ragged.chunks(len(natives)):
        x0, a0, b0, g0 = int(x_off[c0]), int(a_off[c0]), int(b_off[c0]), int(g_off[c0])
        tiles = -(-n[c0:c1] // L.RESAMPLE_CHUNK)
        tab, tab_dev = ragged.table([x_off[c0:c1] - x0, n[c0:c1], a_off[c0:c1] - a0, m[c0:c1], b_off[c0:c1] - b0, mp[c0:c1],
                                     g_off[c0:c1] - g0, J[c0:c1], ragged.offsets(tiles)], device)
        L.check(h.sos_resample_merge_batch_f32(L.ptr(x[x0:]), L.ptr(a[a0:]), L.ptr(b[b0:]), L.ptr(s[g0:]) if s is not None else None,
                                               L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0, ratio, L.ptr(win), win.numel(),
                                               num_table, hop, L.ptr(out[x0:]), L.stream_ptr()), "sos_resample_merge_batch_f32")
    return ragged.split(out, n)
