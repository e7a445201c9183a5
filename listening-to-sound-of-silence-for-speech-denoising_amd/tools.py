"""Mirror of the on-path pieces of the reference `tools.py` (M2/tools.py:217-303,340-362)."""
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


def _host_table(rows, cols):
    tab = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, cols))
    if tab.shape[0] < 1:
        raise ValueError("an empty table")
    return tab


def _upload(host, device):
    from .engine import upload
    return upload(host, torch.int64 if host.dtype == np.int64 else torch.float64, device)


def ragged_stage(flat, table, stride, bits=None, ratios=None):
    """A ragged group staged for the networks in one launch (sos_ragged_stage_f32).  flat: the clips back to back, f32 GPU
    tensor; table: host rows {sample offset, samples, bit offset, frames}, one per clip; bits: the clips' frame decisions back
    to back (uint8 GPU tensor, 1 = non-silent); ratios: samples per frame, one float per clip.
    -> (wave (B, stride), masked (B, stride), mask back to back like `flat`): the clip zero-filled to the stride, clip * mask
    likewise, and the sample mask (1 = silent), each clip's bit for bit bits_to_mask_batch of that clip alone at its ratio.
    Without `bits` only `wave` is computed and returned."""
    L.require_cuda(flat, bits)
    tab = _host_table(table, 4)
    B = tab.shape[0]
    if flat.dim() != 1 or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("flat must be a contiguous 1-D float32 tensor")
    if flat.numel() < int(tab[:, 1].sum()):
        raise ValueError("the table names more samples than `flat` holds")
    wave = torch.empty((B, int(stride)), dtype=torch.float32, device=flat.device)
    d_tab = _upload(tab, flat.device)
    masked = mask = rat = d_rat = None
    if bits is not None:
        if bits.dim() != 1 or bits.dtype != torch.uint8 or not bits.is_contiguous() or bits.numel() < int(tab[:, 3].sum()):
            raise ValueError("bits must be a contiguous 1-D uint8 tensor holding every frame of the table")
        rat = ragged.per_clip(ratios, B, "ratios")
        d_rat = _upload(rat, flat.device)
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
    tab = _host_table(table, 3)
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 (R, stride) tensor")
    out = torch.empty(int(tab[:, 1].sum()), dtype=torch.float32, device=rows.device)
    d_tab = _upload(tab, rows.device)
    L.check(L.lib().sos_ragged_unpack_f32(L.ptr(rows), rows.shape[0], rows.shape[1], L.ptr(d_tab), tab.ctypes.data,
                                          tab.shape[0], L.ptr(out), L.stream_ptr()), "sos_ragged_unpack_f32")
    return out


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


def trim_unknown_frames(bits):
    """M1/tools.py:270-274,306-311 (`truncate`): the first two runs of '2' (unlabelled frames) bound the labelled part
    of a bit-stream; a stream without two such runs is used whole.  Returns (first, end) frame indices.  One helper
    for the file data loader and the on-disk hand-off."""
    from itertools import groupby
    runs = [len(list(g)) for k, g in groupby(bits) if k == '2']
    if len(runs) >= 2:
        return runs[0], len(bits) - runs[1]
    return 0, len(bits)
