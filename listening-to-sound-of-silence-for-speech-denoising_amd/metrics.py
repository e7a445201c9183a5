"""Objective measures of the reference's M2/metrics.py with the same names and arguments:
metrics_L1 (:40-45), metrics_ssnr (:86-130), metrics_ssnr_shift (:132-176), metrics_ssnr_exclude_silence (:178-244),
llr (:561-623), wss (:404-558), CompositeEval (:346-402), evaluate_metrics (:16-33).

The per-sample / per-frame work runs in HIP kernels (csrc/metrics.hip); the per-frame results (a few thousand numbers)
are finalised here on the host exactly like the reference does (log10, clamp, means, the 95 % trimmed means and the
composite regression formulas).

STOI and extended STOI (`stoi`, `stoi_batch`: pystoi's `stoi(x, y, fs_sig, extended)` contract, Taal et al. 2011 and
Jensen & Taal 2016) run in HIP as well (csrc/stoi.hip): resampling to 10 kHz, silent-frame removal, third-octave band
envelopes and the segment correlations of a whole ragged batch in one launch sequence, one synchronisation at the end.
Their float64 restatement is tests/stoi_reference.py; parity against pystoi itself is unpinned (not installed here).
PESQ comes from a third-party package (pypesq) that is absent: `evaluate_metrics` / `CompositeEval` take it, and STOI, as
arguments and return None for everything that depends on a missing one (`handoff.denoise_files(..., stoi_fn=stoi)`
fills in STOI).  SI-SDR (`si_sdr`, `si_sdr_batch`: the formula of the project's parity criterion, oracle/frontend.py::si_sdr) and
the BSS-eval SDR (`sdr`, `sdr_batch`: mir_eval's bss_eval_sources with one source, a 512-tap distortion filter) of ragged batches
run in HIP too (csrc/sdr.hip): float64 sums, lag correlations and Levinson-Durbin solve, one launch sequence per measure;
float64 restatement tests/sdr_reference.py, parity against mir_eval itself unpinned (not installed here).
ITU-R BS.1770 / EBU R128 integrated loudness (`loudness`, `loudness_batch`, `k_weighting`) of ragged batches of multi-channel
files runs in HIP too (csrc/loudness.hip): the K-weighting recurrence as a chunked scan in float64, the two gates on the device,
one launch sequence and no wait; float64 restatement tests/loudness_reference.py, held against the standard's 48 kHz table and
the EBU Tech 3341 signals.  The other R128 measures sit beside it: the true peak by 4x interpolation (`true_peak`,
`true_peak_batch`, `true_peak_filter`), the loudness range and the maximum momentary / short-term loudness
(`loudness_batch(true_peak=, loudness_range=)`); float64 restatement tests/r128_reference.py.
`evaluate_metrics_batch` scores a ragged batch of clips in one launch sequence (csrc/metrics_batch.hip) with the per-frame
arithmetic of the one-clip kernels.  Signals: 1-D numpy arrays or GPU tensors.  No CPU fallback."""
import ctypes as C
import math
import warnings
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib as L
from . import ragged
from .planes import check_planes, plane_frames, planes_flat
from .ragged import device_f32 as _dev

CENT_FREQ = [50., 120, 190, 260, 330, 400, 470, 540, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54,
             1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63]
BANDWIDTH = [70., 70, 70, 70, 70, 70, 70, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154,
             183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136]
_tables = {}


def _num_frames(n, winlength, skip):
    """The reference's frame count, evaluated in f64 as it does (not (n - winlength) // skip), clamped at 0."""
    return max(int(n / skip - (winlength / skip)), 0)


def _wss_n_fft(winlength):
    return int(2 ** np.ceil(np.log(2 * winlength) / np.log(2)))


def _lpc_order(srate):
    return 10 if srate < 10000 else 16


def _frame_setup(n, srate, win_ms=30):
    winlength = int(np.round(win_ms * srate / 1000))
    skip = winlength // 4
    key = ("win", winlength)
    if key not in _tables:
        time = np.linspace(1, winlength, winlength) / (winlength + 1)
        _tables[key] = torch.from_numpy(0.5 * (1 - np.cos(2 * np.pi * time))).cuda()
    return winlength, skip, _num_frames(n, winlength, skip), _tables[key]


def _totals(ref, deg):
    out = torch.empty(3, dtype=torch.float64, device=ref.device)
    L.check(L.lib().sos_metric_totals(L.ptr(ref), L.ptr(deg), ref.numel(), L.ptr(out), L.stream_ptr()), "sos_metric_totals")
    return out.cpu().numpy()


def _frame_energies(ref, deg, srate):
    w, s, nf, win = _frame_setup(ref.numel(), srate)
    if nf < 1:
        return np.zeros((0, 2))
    out = torch.empty((nf, 2), dtype=torch.float64, device=ref.device)
    L.check(L.lib().sos_metric_frame_energy(L.ptr(ref), L.ptr(deg), ref.numel(), w, s, nf, L.ptr(win), L.ptr(out), L.stream_ptr()),
            "sos_metric_frame_energy")
    return out.cpu().numpy()


def _segmental(en, min_snr, max_snr, eps, inner):
    if len(en) == 0:
        return float("nan")
    seg = 10 * np.log10(en[:, 0] / (en[:, 1] + eps) + inner)
    return float(np.nanmean(np.minimum(np.maximum(seg, min_snr), max_snr)))


def _same_length(ref, deg):
    if ref.numel() != deg.numel():
        raise AssertionError(ref.numel())
    return ref, deg


def metrics_L1(output, target):
    o, t = _dev(output), _dev(target)
    res = torch.empty(1, dtype=torch.float64, device=o.device)
    L.check(L.lib().sos_metric_l1(L.ptr(o), o.numel(), L.ptr(t), t.numel(), L.ptr(res), L.stream_ptr()), "sos_metric_l1")
    return float(res.cpu()[0])


def metrics_ssnr(ref_wav, deg_wav, srate=16000, win_len=30, min_snr=-10, max_snr=35, eps=1e-10):
    ref, deg = _same_length(_dev(ref_wav), _dev(deg_wav))
    tot = _totals(ref, deg)
    overall = _overall_snr(tot, eps)
    return overall, _segmental(_frame_energies(ref, deg, srate), min_snr, max_snr, eps, eps)


def metrics_ssnr_shift(ref_wav, deg_wav, srate=16000, win_len=30, min_snr=-10, max_snr=35, eps=1e-10):
    ref, deg = _same_length(_dev(ref_wav), _dev(deg_wav))
    tot = _totals(ref, deg)
    overall = _overall_snr(tot, eps)
    return overall, _segmental(_frame_energies(ref, deg, srate), min_snr, max_snr, eps, 1.0)


def metrics_ssnr_exclude_silence(ref_wav, deg_wav, srate=16000, win_len=30, min_snr=-10, max_snr=35, eps=1e-10):
    ref, deg = _same_length(_dev(ref_wav), _dev(deg_wav))
    tot = _totals(ref, deg)
    overall = _overall_snr(tot, eps)
    nc, npz = torch.empty_like(ref), torch.empty_like(deg)
    cnt = torch.zeros(1, dtype=torch.int64, device=ref.device)
    thr = np.float32(np.float32(tot[2]) * np.float32(0.03))
    L.check(L.lib().sos_metric_compact(L.ptr(ref), L.ptr(deg), ref.numel(), float(thr), L.ptr(nc), L.ptr(npz), L.ptr(cnt),
                                       L.stream_ptr()), "sos_metric_compact")
    k = int(cnt.cpu()[0])
    return overall, _segmental(_frame_energies(nc[:k].contiguous(), npz[:k].contiguous(), srate), min_snr, max_snr, eps, eps)


def llr(ref_wav, deg_wav, srate):
    ref, deg = _same_length(_dev(ref_wav), _dev(deg_wav))
    w, s, nf, win = _frame_setup(ref.numel(), srate)
    out = torch.empty(max(nf, 1), dtype=torch.float32, device=ref.device)
    if nf:
        L.check(L.lib().sos_metric_llr(L.ptr(ref), L.ptr(deg), ref.numel(), w, s, nf, L.ptr(win), _lpc_order(srate), L.ptr(out),
                                       L.stream_ptr()), "sos_metric_llr")
    return out[:nf].cpu().numpy()


def _crit_filters(srate, n_fft, device):
    key = ("crit", srate, n_fft, str(device))
    if key not in _tables:
        half = n_fft // 2
        max_freq = srate / 2
        min_factor = np.exp(-30. / (2 * 2.303))
        j = np.arange(half)
        cf = np.zeros((25, half))
        for i in range(25):
            f0 = np.floor((CENT_FREQ[i] / max_freq) * half)
            bw = (BANDWIDTH[i] / max_freq) * half
            row = np.exp(-11 * (((j - f0) / bw) ** 2) + np.log(BANDWIDTH[0]) - np.log(BANDWIDTH[i]))
            cf[i] = row * (row > min_factor)
        _tables[key] = torch.from_numpy(cf.astype(np.float32)).to(device)
    return _tables[key]


def wss(ref_wav, deg_wav, srate, eps=1e-10):
    ref, deg = _same_length(_dev(ref_wav), _dev(deg_wav))
    w, s, nf, win = _frame_setup(ref.numel(), srate)
    n_fft = _wss_n_fft(w)
    out = torch.empty(max(nf, 1), dtype=torch.float32, device=ref.device)
    if nf:
        cf = _crit_filters(srate, n_fft, ref.device)
        L.check(L.lib().sos_metric_wss(L.ptr(ref), L.ptr(deg), ref.numel(), w, s, nf, L.ptr(win), n_fft, L.ptr(cf), float(eps),
                                       L.ptr(out), L.stream_ptr()), "sos_metric_wss")
    return [float(v) for v in out[:nf].cpu().numpy()]


def _overall_snr(tot, eps):
    return float(10 * np.log10(tot[0] / (tot[1] + eps)))


def _composite(wss_frames, llr_frames, segSNR, overall_snr, pesq_raw):
    """The reference's composite measures from the per-frame WSS (list of floats) and LLR (f32 array) values: the two
    sorted 95 % trimmed means and the regressions of M2/metrics.py:377-402."""
    wv = sorted(wss_frames)
    wss_dist = float(np.nanmean(wv[:int(round(len(wv) * 0.95))]))
    lv = sorted(llr_frames)
    llr_mean = float(np.nanmean(lv[:round(len(lv) * 0.95)]))
    if pesq_raw is None:
        return None, None, None, None, segSNR, overall_snr

    def trim_mos(val):
        return min(max(val, 1), 5)
    Csig = trim_mos(3.093 - 1.029 * llr_mean + 0.603 * pesq_raw - 0.009 * wss_dist)
    Cbak = trim_mos(1.634 + 0.478 * pesq_raw - 0.007 * wss_dist + 0.063 * segSNR)
    Covl = trim_mos(1.594 + 0.805 * pesq_raw - 0.512 * llr_mean - 0.007 * wss_dist)
    return Csig, Cbak, Covl, pesq_raw, segSNR, overall_snr


def CompositeEval(ref_wav, deg_wav, srate=16000, eps=1e-10, pesq_raw=None):
    """(Csig, Cbak, Covl, pesq_raw, segSNR, overall_snr); the first four are None without a PESQ value
    (the reference calls pypesq here, M2/metrics.py:377)."""
    ref, deg = _dev(ref_wav), _dev(deg_wav)
    n = min(ref.numel(), deg.numel())
    ref, deg = ref[:n].contiguous(), deg[:n].contiguous()
    wv = wss(ref, deg, srate, eps=eps)
    lv = llr(ref, deg, srate)
    overall_snr, segSNR = metrics_ssnr(ref, deg, srate=srate, min_snr=0, eps=eps)
    return _composite(wv, lv, segSNR, overall_snr, pesq_raw)


def evaluate_metrics(noisy, clean, sr=16000, eps=1e-20, pesq=None, stoi=None):
    """Same keys and order as the reference (M2/metrics.py:16-33); `pesq` / `stoi`: values computed elsewhere
    (pypesq.pesq(clean, noisy, sr); stoi(clean, noisy, sr) of this module or pystoi's) or None."""
    csig, cbak, covl, pesq_raw, ssnr, overall_snr = CompositeEval(clean, noisy, sr, eps=eps, pesq_raw=pesq)
    m = OrderedDict()
    m['l1'] = metrics_L1(noisy, clean)
    m['stoi'] = stoi
    m['csig'], m['cbak'], m['covl'], m['pesq'] = csig, cbak, covl, pesq_raw
    m['ssnr_regular'] = metrics_ssnr(clean, noisy, srate=sr, eps=eps)[1]
    m['ssnr_shift'] = metrics_ssnr_shift(clean, noisy, srate=sr, eps=eps)[1]
    m['ssnr_clip'] = ssnr
    m['ssnr_exsi'] = metrics_ssnr_exclude_silence(clean, noisy, srate=sr, eps=eps)[1]
    m['overall_snr'] = overall_snr
    return m


# ---- ragged batches of clip pairs: the driver under evaluate_metrics_batch, stoi_batch, si_sdr_batch and sdr_batch
_BATCH_HEAD = 8                     # f64 per clip at the front of sos_metric_batch's packed output (include/sos_hip.h)
# One launch sequence's worth of pairs: the concatenated device buffers x / y, the host lengths `lens` (int64), the device
# table `tab` = [offsets, lengths] and `lead` = (x, y, offsets, lengths, lengths_host, nclips), the arguments every
# sos_*_batch entry point starts with.
_Chunk = namedtuple("_Chunk", "x y lens tab lead")


def _check_pairs(a, b, counted, named, allow_empty=False):
    """The two lists of signals as lists, after the checks every batch entry point makes: as many of one as of the other, each
    pair of one shape and (unless allow_empty) no empty clip.  counted / named: what the messages call the two sides."""
    a, b = list(a), list(b)
    if len(a) != len(b):
        raise ValueError(f"{len(a)} {counted[0]} but {len(b)} {counted[1]}")
    for i, (x, y) in enumerate(zip(a, b)):
        if tuple(np.shape(x)) != tuple(np.shape(y)):
            raise ValueError(f"clip {i}: {named[0]} and {named[1]} should have the same length, found {tuple(np.shape(x))} and "
                             f"{tuple(np.shape(y))}")
        if not allow_empty and int(np.prod(np.shape(x))) == 0:
            raise ValueError(f"clip {i} is empty")
    return a, b


def _chunks(a, b):
    """The pairs (a[i], b[i]) as _Chunks of at most ragged.MAX_CLIPS clips, each uploaded when it is asked for."""
    for c0 in range(0, len(a), ragged.MAX_CLIPS):
        x, n = ragged.concat(a[c0:c0 + ragged.MAX_CLIPS])
        y, _ = ragged.concat(b[c0:c0 + ragged.MAX_CLIPS])
        lens = np.asarray(n, dtype=np.int64)
        tab = torch.from_numpy(np.stack([ragged.offsets(lens), lens])).to(x.device)
        lead = (L.ptr(x), L.ptr(y), L.ptr(tab[0]), L.ptr(tab[1]), lens.ctypes.data_as(C.c_void_p), len(lens))
        yield _Chunk(x, y, lens, tab, lead)


def _workspace(sizer, ch, *params):
    """The device workspace the library's function `sizer` (a sos_*_workspace_bytes) asks for the chunk's lengths."""
    nbytes = getattr(L.lib(), sizer)(ch.lead[4], ch.lead[5], *params)
    if nbytes < 0:
        L.check(-22, sizer)
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=ch.x.device)


def _per_clip(values, nclips, name):
    if values is None:
        return [None] * nclips
    values = list(values)
    if len(values) != nclips:
        raise ValueError(f"{len(values)} {name} values for {nclips} clips")
    return values


def evaluate_metrics_batch(noisy, clean, sr=16000, eps=1e-20, pesq=None, stoi=None, return_detail=False, si_sdr=False, sdr=False):
    """evaluate_metrics of every pair (noisy[i], clean[i]) of 1-D signals (numpy arrays or GPU tensors; any lengths, each pair
    equal): a list with one OrderedDict per clip, the same keys, order and meaning.  The whole batch goes up once, runs as
    one launch sequence (csrc/metrics_batch.hip) and comes back in one copy; a clip's values depend on that clip's samples
    only, so it gets the same bits alone, in any batch and in any order.  `pesq` / `stoi`: None or one value per clip (entries
    may be None); stoi=True computes stoi_batch(clean, noisy, sr).  return_detail=True returns (results, detail) with, per
    clip, the frame count, the kept-sample and kept-frame counts of the silence rule (computed on the device) and the
    per-frame LLR, WSS and frame-energy arrays.  si_sdr=True / sdr=True append the keys 'si_sdr' / 'sdr' after 'overall_snr':
    si_sdr_batch / sdr_batch of (clean[i], noisy[i]), their launch sequences enqueued before the call's one wait."""
    noisy, clean = _check_pairs(noisy, clean, ("noisy signals", "clean ones"), ("noisy", "clean"))
    nclips = len(clean)
    pesq = _per_clip(pesq, nclips, "pesq")
    stoi = stoi_batch(clean, noisy, sr) if stoi is True else _per_clip(stoi, nclips, "stoi")
    results, detail = [], []
    if nclips == 0:
        return (results, detail) if return_detail else results
    outs, plans, base = [], [], 0
    for ch in _chunks(clean, noisy):
        lens = ch.lens
        w, skip, _, win = _frame_setup(int(lens[0]), sr)
        frames = np.asarray([_num_frames(int(v), w, skip) for v in lens], dtype=np.int64)
        n_fft = _wss_n_fft(w)
        cf = _crit_filters(sr, n_fft, ch.x.device)
        ws = _workspace("sos_metric_batch_workspace_bytes", ch, w, skip, n_fft)
        ftot = int(frames.sum())
        out = torch.empty(8 * _BATCH_HEAD * len(lens) + 40 * ftot, dtype=torch.uint8, device=ch.x.device)
        L.check(L.lib().sos_metric_batch(*ch.lead, w, skip, n_fft, _lpc_order(sr), L.ptr(win), L.ptr(cf), float(eps), L.ptr(ws),
                                         ws.numel(), L.ptr(out), out.numel(), L.stream_ptr()), "sos_metric_batch")
        outs.append(out)
        extra, pos = [], base + out.numel()          # (key, byte offset in the one copy) of the optional measures
        for key, on, fl in (("si_sdr", si_sdr, None), ("sdr", sdr, SDR_FILTER_LENGTH)):
            if on:
                outs.append(_sdr_enqueue(ch, fl).view(torch.uint8).reshape(-1))
                extra.append((key, pos))
                pos += outs[-1].numel()
        plans.append((base, lens, frames, ftot, extra))
        base = pos
    buf = (outs[0] if len(outs) == 1 else torch.cat(outs)).cpu().numpy()          # the one wait of the call
    i = 0
    for base, lens, frames, ftot, extra in plans:
        nb = len(lens)
        more = OrderedDict()
        for key, o in extra:
            w = _SDR_OUT[key]
            rows = np.frombuffer(buf, np.float64, w * nb, o).reshape(nb, w)
            more[key] = _si_sdr_finish(rows, lens) if key == "si_sdr" else _sdr_finish(rows, lens, i)[0]
        head = np.frombuffer(buf, np.float64, _BATCH_HEAD * nb, base).reshape(nb, _BATCH_HEAD)
        o = base + 8 * _BATCH_HEAD * nb
        energy = np.frombuffer(buf, np.float64, 2 * ftot, o).reshape(ftot, 2)
        energy_kept = np.frombuffer(buf, np.float64, 2 * ftot, o + 16 * ftot).reshape(ftot, 2)
        llr_all = np.frombuffer(buf, np.float32, ftot, o + 32 * ftot)
        wss_all = np.frombuffer(buf, np.float32, ftot, o + 36 * ftot)
        f_off = ragged.offsets(frames)
        for b in range(nb):
            tot, nf, f0 = head[b], int(frames[b]), int(f_off[b])
            if tot[7] < 0 or int(tot[6]) != nf:
                raise RuntimeError("sos_metric_batch: device lengths disagree with the host's")
            k, kf = int(tot[4]), int(tot[5])
            en, ek = energy[f0:f0 + nf], energy_kept[f0:f0 + kf]
            lv, wv = llr_all[f0:f0 + nf], wss_all[f0:f0 + nf]
            overall_snr = _overall_snr(tot, eps)
            ssnr = _segmental(en, 0, 35, eps, eps)
            csig, cbak, covl, pesq_raw, ssnr, overall_snr = _composite([float(v) for v in wv], lv, ssnr, overall_snr, pesq[i])
            m = OrderedDict()
            m['l1'] = float(tot[3] / float(lens[b]))
            m['stoi'] = stoi[i]
            m['csig'], m['cbak'], m['covl'], m['pesq'] = csig, cbak, covl, pesq_raw
            m['ssnr_regular'] = _segmental(en, -10, 35, eps, eps)
            m['ssnr_shift'] = _segmental(en, -10, 35, eps, 1.0)
            m['ssnr_clip'] = ssnr
            m['ssnr_exsi'] = _segmental(ek, -10, 35, eps, eps)
            m['overall_snr'] = overall_snr
            for key, vals in more.items():
                m[key] = vals[b]
            results.append(m)
            if return_detail:
                detail.append(dict(frames=nf, kept_samples=k, kept_frames=kf, llr=lv.copy(), wss=wv.copy(), energy=en.copy(),
                                   energy_kept=ek.copy()))
            i += 1
    return (results, detail) if return_detail else results


# ---- STOI / extended STOI (pystoi's constants: 10 kHz, 256-sample frames at hop 128, 15 third-octave bands from 150 Hz,
# 30-frame segments, clipping at BETA = -15 dB, 40 dB dynamic range)
STOI_FS = 10000
STOI_NUMBAND = 15


def _stoi_ratio(fs_sig):
    if isinstance(fs_sig, bool) or int(fs_sig) != fs_sig or fs_sig <= 0:
        raise ValueError(f"fs_sig must be a positive integer sample rate, got {fs_sig!r}")
    g = math.gcd(STOI_FS, int(fs_sig))
    return STOI_FS // g, int(fs_sig) // g


def _stoi_taps(p, q, device):
    """pystoi's resample_oct filter (a port of Octave's resample): fc = 1/(2 max(p,q)), roll-off fc/10, 60 dB rejection,
    Kaiser window; normalised to unit sum and scaled by p, as scipy.signal.resample_poly applies it."""
    key = ("stoi", p, q, str(device))
    if key not in _tables:
        fc = 1. / (2 * max(p, q))
        L_ = int(np.ceil((60. - 8) / (28.714 * (fc / 10))))
        t = np.arange(-L_, L_ + 1)
        h = np.kaiser(2 * L_ + 1, 0.1102 * (60. - 8.7)) * (2 * p * fc * np.sinc(2 * fc * t))
        _tables[key] = torch.from_numpy(h / h.sum() * p).to(device)
    return _tables[key]


def stoi_batch(clean, processed, fs_sig, extended=False, return_frames=False):
    """STOI (or, extended=True, ESTOI) of every pair (clean[i], processed[i]) of 1-D signals sampled at fs_sig; the
    clips may have any lengths, each pair equal.  One launch sequence for the whole batch and one synchronisation at the
    end; a clip's score does not depend on the other clips of the batch.  A clip with fewer than 30 STFT frames after
    silent-frame removal scores 1e-5 with a RuntimeWarning, as pystoi does.  Returns the list of scores, or
    (scores, kept-frame counts) with return_frames=True."""
    clean, processed = _check_pairs(clean, processed, ("clean signals", "processed ones"), ("x", "y"), allow_empty=True)
    p, q = _stoi_ratio(fs_sig)
    scores, frames = [], []
    if not clean:
        return (scores, frames) if return_frames else scores
    outs = []
    for ch in _chunks(clean, processed):
        taps = _stoi_taps(p, q, ch.x.device) if p != q else None
        ws = _workspace("sos_stoi_workspace_bytes", ch, p, q)
        out = torch.empty((len(ch.lens), 3), dtype=torch.float64, device=ch.x.device)
        L.check(L.lib().sos_stoi_batch(*ch.lead, p, q, L.ptr(taps), 0 if taps is None else taps.numel(), int(bool(extended)),
                                       L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()), "sos_stoi_batch")
        outs.append(out)
    res = torch.cat(outs).cpu().numpy()
    for total, segments, kept in res:
        if kept < 0:
            raise RuntimeError("sos_stoi_batch: device lengths disagree with the host's")
        frames.append(int(kept))
        if segments == 0:
            warnings.warn("Not enough STFT frames to compute intermediate intelligibility measure after removing silent "
                          "frames. Returning 1e-5. Please check you wav files", RuntimeWarning)
            scores.append(1e-5)
        else:
            scores.append(float(total / (segments * (1 if extended else STOI_NUMBAND))))
    return (scores, frames) if return_frames else scores


def stoi(x, y, fs_sig, extended=False):
    """pystoi's stoi(x, y, fs_sig, extended=False): x clean, y processed (1-D, same shape), fs_sig in Hz -> float.
    stoi_batch of one clip."""
    if tuple(np.shape(x)) != tuple(np.shape(y)):
        raise ValueError(f"x and y should have the same length, found {tuple(np.shape(x))} and {tuple(np.shape(y))}")
    return stoi_batch([x], [y], fs_sig, extended)[0]


# ---- SI-SDR and the BSS-eval SDR (csrc/sdr.hip)
SDR_FILTER_LENGTH = 512             # mir_eval's bss_eval_sources: taps of the allowed distortion filter; the kernels' maximum
_SDR_OUT = {"si_sdr": 4, "sdr": 5}  # f64 per clip of sos_sisdr_batch / sos_sdr_batch (include/sos_hip.h)


def _sdr_enqueue(ch, filter_length=None, zero_mean=False, stages=L.SDR_CORRELATE | L.SDR_SOLVE, ws=None):
    """Enqueue sos_sisdr_batch (filter_length None) or sos_sdr_batch on the _Chunk `ch` of (clean, estimate) pairs; no wait.
    Returns the f64 [clips][4] or [clips][5] device result (include/sos_hip.h).  `stages` / `ws`: one part of the SDR sequence on
    a workspace the caller keeps (tools/sdr_bench.py times the correlation and the solve apart)."""
    h, si = L.lib(), filter_length is None
    if ws is None:
        ws = _workspace("sos_sdr_workspace_bytes", ch, 0 if si else int(filter_length))
    out = torch.empty((len(ch.lens), _SDR_OUT["si_sdr" if si else "sdr"]), dtype=torch.float64, device=ch.x.device)
    if si:
        L.check(h.sos_sisdr_batch(*ch.lead, int(bool(zero_mean)), L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()),
                "sos_sisdr_batch")
    else:
        L.check(h.sos_sdr_batch(*ch.lead, int(filter_length), int(stages), L.ptr(ws), ws.numel(), L.ptr(out), L.stream_ptr()),
                "sos_sdr_batch")
    return out


def _si_sdr_finish(rows, lens):
    """Scores from sos_sisdr_batch's rows {sum (alpha x)^2, sum (alpha x - y)^2, alpha, samples}."""
    if np.any(rows[:, 3] != lens):
        raise RuntimeError("sos_sisdr_batch: device lengths disagree with the host's")
    return [float(10.0 * np.log10((t + 1e-30) / (r + 1e-30))) for t, r in rows[:, :2]]


def _sdr_finish(rows, lens, first_clip=0):
    """(scores, detail) from sos_sdr_batch's rows {p, e, r[0], status, samples}: 10 log10(p / (e - p)) in float64; nan with a
    RuntimeWarning where the clean clip is all zero or the recursion failed, inf where e - p <= 0."""
    if np.any(rows[:, 4] != lens):
        raise RuntimeError("sos_sdr_batch: device lengths disagree with the host's")
    scores, detail = [], []
    for b, (p, e, r0, status, _) in enumerate(rows):
        detail.append(dict(p=float(p), e=float(e), r0=float(r0), status=int(status)))
        if status < 0:
            why = "the clean signal is all zero" if status == -2 else "the lag matrix of the clean signal is numerically singular"
            warnings.warn(f"sdr: clip {first_clip + b}: {why}. Returning nan", RuntimeWarning)
            scores.append(float("nan"))
        elif e - p <= 0:
            scores.append(float("inf"))
        else:
            with np.errstate(divide="ignore"):
                scores.append(float(10.0 * np.log10(p / (e - p))))
    return scores, detail


def _sdr_run(clean, estimate, key, filter_length=None, zero_mean=False):
    """The f64 result rows and host lengths of the whole batch: the pairs checked, one launch sequence per 65535 clips, one wait."""
    clean, estimate = _check_pairs(clean, estimate, ("clean signals", "estimates"), ("clean", "estimate"))
    outs, lens_all = [], []
    for ch in _chunks(clean, estimate):
        outs.append(_sdr_enqueue(ch, filter_length, zero_mean))
        lens_all.append(ch.lens)
    rows = (outs[0] if len(outs) == 1 else torch.cat(outs)).cpu().numpy() if outs else np.zeros((0, _SDR_OUT[key]))
    return rows, np.concatenate(lens_all) if lens_all else np.zeros(0, np.int64)


def si_sdr_batch(clean, estimate, zero_mean=False):
    """Scale-invariant SDR in dB of every pair (clean[i], estimate[i]) of 1-D signals (numpy arrays or GPU tensors; any
    lengths, each pair equal): oracle/frontend.py::si_sdr(est=estimate, ref=clean) with its 1e-30 terms, alpha =
    <y,x> / (<x,x> + 1e-30), 10 log10((|alpha x|^2 + 1e-30) / (|alpha x - y|^2 + 1e-30)); zero_mean=True removes each
    signal's mean first.  Float64 sums on the device, one launch sequence and one wait for the batch; a clip's value does not
    depend on the other clips.  Returns the list of floats."""
    return _si_sdr_finish(*_sdr_run(clean, estimate, "si_sdr", None, zero_mean))


def si_sdr(clean, estimate, zero_mean=False):
    """si_sdr_batch of one clip."""
    return si_sdr_batch([clean], [estimate], zero_mean)[0]


def sdr_batch(clean, estimate, filter_length=SDR_FILTER_LENGTH, return_detail=False):
    """BSS-eval SDR in dB (Vincent et al. 2006; mir_eval.separation.bss_eval_sources with one source) of every pair
    (clean[i], estimate[i]): the energy of the estimate's projection on the `filter_length` (1 .. 512) delayed copies of the
    clean signal over the energy of the rest.  With r[k] = sum_t x[t] x[t+k], d[k] = sum_t x[t] y[t+k], toeplitz(r) c = d,
    p = d.c and e = sum y^2 (all float64 on the device) it is 10 log10(p / (e - p)).  An all-zero clean clip (or a lag matrix
    the recursion finds singular) scores nan with a RuntimeWarning naming the clip; an estimate inside the span up to rounding
    (e - p <= 0) scores inf.  One launch sequence and one wait for the batch; a clip's value does not depend on the other clips.
    Returns the list of floats, or (scores, detail) with per clip dict(p, e, r0, status) when return_detail=True."""
    if isinstance(filter_length, bool) or int(filter_length) != filter_length or not 1 <= filter_length <= SDR_FILTER_LENGTH:
        raise ValueError(f"filter_length must be an integer in 1 .. {SDR_FILTER_LENGTH}, got {filter_length!r}")
    scores, detail = _sdr_finish(*_sdr_run(clean, estimate, "sdr", int(filter_length)))
    return (scores, detail) if return_detail else scores


def sdr(clean, estimate, filter_length=SDR_FILTER_LENGTH, return_detail=False):
    """sdr_batch of one clip."""
    res = sdr_batch([clean], [estimate], filter_length, return_detail)
    return (res[0][0], res[1][0]) if return_detail else res[0]


# ---- ITU-R BS.1770 / EBU R128 integrated loudness (csrc/loudness.hip)
LOUDNESS_SPLIT = 8                  # chunks per 100 ms hop of the filter scan (1 .. 64, at most the hop): short files fill more lanes
LOUDNESS_COLS = 8                   # int64 per file of the table (include/sos_hip.h: sos_loudness_batch_f64)


def k_weighting(sr):
    """The K-weighting filter of ITU-R BS.1770 at `sr` Hz: float64 [10] = {b0, b1, b2, a1, a2} of the high shelf, then of the
    high-pass (a0 = 1), from the closed forms libebur128 uses; at 48 kHz the standard's table to 1e-12."""
    sr = float(sr)
    if not math.isfinite(sr) or sr <= 0:
        raise ValueError("k_weighting: the rate is a positive number of Hz, got %r" % (sr,))
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return np.asarray(shelf + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)


def loudness_hop(sr):
    """Samples of a 100 ms hop at `sr` Hz as libebur128 rounds it; a gating block is four hops."""
    return (int(sr) + 5) // 10


def loudness_table(chans, avail, frames, hops, split=LOUDNESS_SPLIT):
    """The host table of sos_loudness_batch_f64 / sos_loudness_gain_batch_f32 for files whose planes lie back to back: int64
    [files][8] = {first plane sample, plane length, channels, frames, 0, hop, first weight, first chunk}."""
    chans, avail, frames, hops = (np.asarray(v, dtype=np.int64) for v in (chans, avail, frames, hops))
    chunks = chans * -(-frames // np.maximum(hops, 1)) * split
    return np.ascontiguousarray(np.stack([ragged.offsets(chans * avail), avail, chans, frames, np.zeros_like(chans), hops,
                                          ragged.offsets(chans), ragged.offsets(chunks)], axis=1), dtype=np.int64)


def _loudness_weights(channel_weights, planes, who):
    """One float64 weight per channel of every file, files in order (1.0 where the caller gives none)."""
    if channel_weights is None:
        channel_weights = [None] * len(planes)
    channel_weights = list(channel_weights)
    if len(channel_weights) != len(planes):
        raise ValueError("%s: channel_weights holds one entry per file (%d files, %d entries)" % (who, len(planes), len(channel_weights)))
    out = []
    for i, (w, p) in enumerate(zip(channel_weights, planes)):
        w = np.ones(p.shape[0]) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
        if w.size != p.shape[0] or not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("%s: file %d has %d channels and needs as many finite weights >= 0, got %r" % (who, i, p.shape[0], w.tolist()))
        out.append(w)
    return out


TRUE_PEAK_TILE = 2048               # points of one plane per tile of sos_true_peak_batch_f64: TP_TILE of csrc/loudness.hip, which
                                    # tests/test_r128_reference.py holds it to


def true_peak_filter():
    """The true-peak interpolator's coefficients, float32 [3][12]: h_p[k] = sinc(u) I0(9 sqrt(1 - (u / 6)^2)) / I0(9) with u = k -
    p / 4 for the phases p = 1, 2, 3 and the taps k = -5 .. 6 (4x oversampling by a 48-tap Kaiser-windowed sinc), computed in
    float64 and rounded once.  Phase 0 is the sample itself: the prototype is 0 at every other whole sample."""
    u = np.arange(-5, 7, dtype=np.float64)[None, :] - np.arange(1, 4, dtype=np.float64)[:, None] / 4.0
    return np.ascontiguousarray(np.sinc(u) * np.i0(9.0 * np.sqrt(1.0 - (u / 6.0) ** 2)) / np.i0(9.0), dtype=np.float32)


def _true_peaks(planes_flat_of, frames, device):
    """sos_true_peak_batch_f64 over a checked, non-empty batch: (flat, src, chans, avail) -> f64 [files] on the device."""
    flat, src, chans, avail = planes_flat_of
    from .engine import upload                                       # ragged.upload carries int64 / float64 only
    coef = upload(true_peak_filter(), torch.float32, device)
    peaks = torch.empty(len(chans), dtype=torch.float64, device=device)
    h = L.lib()
    for c0, c1 in ragged.chunks(len(chans)):
        tab = loudness_table(chans[c0:c1], avail[c0:c1], frames[c0:c1], np.ones(c1 - c0, dtype=np.int64), 1)
        tab_dev = ragged.upload(tab, device)
        L.check(h.sos_true_peak_batch_f64(L.ptr(flat[int(src[c0]):]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0,
                                          L.ptr(coef), L.ptr(peaks[c0:]), L.stream_ptr()), "sos_true_peak_batch_f64")
    return peaks


def true_peak_batch(planes, frames=None):
    """The TRUE PEAK (ITU-R BS.1770-4 Annex 2, by the project's own interpolator) of every file of a ragged batch, as a linear
    value: planes and frames as loudness_batch takes them, no rate.  4x oversampling by true_peak_filter(): the point n + p / 4
    is sum_k h_p[k] x[n + k] (12 fmaf in tap order, float32) for n = -1 .. frames - 1, the samples read 0 outside the extent the
    encode reads; the result is the maximum of |x| and of |point| over all channels, never below the sample peak.  -> f64
    [files] STILL ON THE DEVICE, 0 for a file without a sample.  One launch sequence per 65535 files (sos_true_peak_batch_f64),
    no wait; a maximum has no order, so two calls give equal bits.  Float64 restatement: tests/r128_reference.py.
    ValueError before any launch: a file that is not a (1 .. 64 channels, n) float32 tensor, bad frames."""
    who = "true_peak_batch"
    planes = check_planes(who, planes)
    frames = plane_frames(who, planes, frames)
    L.require_cuda(*planes)
    if not planes:
        return torch.zeros(0, dtype=torch.float64, device="cuda")
    return _true_peaks(planes_flat(planes), frames, planes[0].device)


def _one_clip(who, x):
    """x 1-D or (channels, n), a numpy array or a GPU tensor, as one (channels, n) f32 GPU tensor."""
    if np.ndim(x) not in (1, 2):
        raise ValueError("%s: x is 1-D or (channels, n), got %d dimensions" % (who, np.ndim(x)))
    if torch.is_tensor(x):
        L.require_cuda(x)
        y = x.detach().float().contiguous()
    elif not torch.cuda.is_available():
        raise RuntimeError("sos_amd.metrics needs an MI355X: there is no CPU fallback")
    else:
        y = torch.from_numpy(np.array(x, dtype=np.float32, order="C")).cuda()
    return y.reshape(1, -1) if y.dim() == 1 else y.contiguous()


def true_peak(x):
    """true_peak_batch of one clip: x 1-D or (channels, n), a numpy array or a GPU tensor -> a Python float (one wait)."""
    return float(true_peak_batch([_one_clip("true_peak", x)]).cpu()[0])


def loudness_batch(planes, rates, channel_weights=None, frames=None, split=LOUDNESS_SPLIT, true_peak=False, loudness_range=False):
    """Integrated loudness (ITU-R BS.1770-4 / EBU R128, gated) of every file of a ragged batch.  planes: one (channels, n) f32
    GPU tensor per file, 1 .. 64 channels; rates: its sample rate in Hz (one per file, or one for all); channel_weights: per file
    None (every channel counts 1.0: exact for mono and stereo) or one weight >= 0 per channel (surround: 1.41 for the rear pair,
    0 for the LFE -- the caller's to pass); frames: samples per channel that count, per file (default n; past n the file reads
    0, below n it is cropped: what encode_batch_device writes).
    Per channel the K-weighting filter (k_weighting(rate), zero state, float64); blocks of 4 h samples every h = (rate + 5) // 10,
    whole blocks only; z = sum over channels of weight * mean square; l = -0.691 + 10 log10 z; the absolute gate l > -70, the
    relative gate l > (loudness of the absolutely gated blocks) - 10; L = -0.691 + 10 log10(mean z of the blocks passing both),
    -inf when none passes.  -> dict of per-file tensors STILL ON THE DEVICE: lufs (f64), peak (f64: max |x| over all channels and
    frames, the SAMPLE peak, not the true peak), blocks / blocks_abs (int64: blocks passing both gates / the absolute one) and
    rows (f64 [files][4], what audio_io.loudness_gain_batch_device reads).  One launch sequence per 65535 files
    (sos_loudness_batch_f64), no wait.  `split`: chunks per hop of the filter scan; it moves the result by rounding only.
    true_peak=True adds the keys true_peak (f64: true_peak_batch of the same planes and frames, one more launch sequence) and
    rows_true (rows with column 1 replaced by it: handed to audio_io.loudness_gain_batch_device, the ceiling then bounds the
    TRUE peak).  loudness_range=True adds lra (f64, LU: EBU Tech 3342 -- short-term windows of 30 hops every hop, gates l > -70
    and l > (loudness of the mean z of the absolutely gated windows) - 20, the 95th minus the 10th nearest-rank percentile of
    the survivors, 0 without one), max_momentary / max_short_term (f64, LUFS: the ungated maxima over the 400 ms blocks / the
    3 s windows, -inf without one) and windows (int64: windows passing both gates), from the chunk energies the measurement
    left on the device (sos_loudness_range_batch_f64, two more launches).  With both False the launches and the keys are the
    ones above.  Float64 restatement of both: tests/r128_reference.py.
    ValueError before any launch: a file that is not such a tensor, a rate below 10 * split Hz, bad weights or frames."""
    who = "loudness_batch"
    planes = check_planes(who, planes)
    rates = [rates] * len(planes) if np.ndim(rates) == 0 else list(rates)
    if len(rates) != len(planes):
        raise ValueError("%s: one rate per file (%d files, %d rates)" % (who, len(planes), len(rates)))
    if isinstance(split, bool) or int(split) != split or not 1 <= split <= 64:
        raise ValueError("%s: split is a whole number within 1 .. 64, got %r" % (who, split))
    for i, r in enumerate(rates):
        if isinstance(r, bool) or int(r) != r or not split <= loudness_hop(r) <= 1 << 31:
            raise ValueError("%s: file %d has the rate %r (a whole number of Hz, its 100 ms hop at least %d samples)" % (who, i, r, split))
    weights = _loudness_weights(channel_weights, planes, who)
    frames = plane_frames(who, planes, frames)
    L.require_cuda(*planes)
    peaks = more = None
    if not planes:
        rows = torch.zeros((0, 4), dtype=torch.float64, device="cuda")
        peaks, more = rows[:, 1], rows
    else:
        device = planes[0].device
        flat, src, chans, avail = planes_flat(planes)
        coef = ragged.upload(np.stack([k_weighting(r) for r in rates]), device)
        rows = torch.empty((len(planes), 4), dtype=torch.float64, device=device)
        if true_peak:
            peaks = _true_peaks((flat, src, chans, avail), frames, device)
        if loudness_range:
            more = torch.empty((len(planes), 4), dtype=torch.float64, device=device)
        h = L.lib()
        for c0, c1 in ragged.chunks(len(planes)):
            tab = loudness_table(chans[c0:c1], avail[c0:c1], frames[c0:c1], [loudness_hop(r) for r in rates[c0:c1]], int(split))
            need = h.sos_loudness_workspace_bytes(tab.ctypes.data_as(C.c_void_p), c1 - c0, int(split))
            if need < 0:
                L.check(-22, "sos_loudness_workspace_bytes")
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            w, tab_dev = ragged.upload(np.concatenate(weights[c0:c1]), device), ragged.upload(tab, device)
            L.check(h.sos_loudness_batch_f64(L.ptr(flat[int(src[c0]):]), L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0,
                                             L.ptr(coef[c0:]), L.ptr(w), int(split), L.ptr(ws), ws.numel(), L.ptr(rows[c0:]),
                                             L.stream_ptr()), "sos_loudness_batch_f64")
            if loudness_range:
                need = h.sos_loudness_range_workspace_bytes(tab.ctypes.data_as(C.c_void_p), c1 - c0)
                if need < 0:
                    L.check(-22, "sos_loudness_range_workspace_bytes")
                rw = torch.empty(need, dtype=torch.uint8, device=device)
                L.check(h.sos_loudness_range_batch_f64(L.ptr(tab_dev), tab.ctypes.data_as(C.c_void_p), c1 - c0, L.ptr(w), int(split),
                                                       L.ptr(ws), ws.numel(), L.ptr(rw), rw.numel(), L.ptr(more[c0:]),
                                                       L.stream_ptr()), "sos_loudness_range_batch_f64")
    out = dict(lufs=rows[:, 0], peak=rows[:, 1], blocks=rows[:, 2].to(torch.int64), blocks_abs=rows[:, 3].to(torch.int64), rows=rows)
    if true_peak:
        rows_true = rows.clone()
        rows_true[:, 1] = peaks
        out.update(true_peak=peaks, rows_true=rows_true)
    if loudness_range:
        out.update(lra=more[:, 0], max_momentary=more[:, 1], max_short_term=more[:, 2], windows=more[:, 3].to(torch.int64))
    return out


def loudness(x, sr, channel_weights=None, true_peak=False, loudness_range=False):
    """loudness_batch of one clip: x 1-D or (channels, n), a numpy array or a GPU tensor -> dict(lufs, peak, blocks, blocks_abs)
    of Python numbers (one wait); with true_peak also true_peak, with loudness_range also lra, max_momentary, max_short_term and
    windows."""
    r = loudness_batch([_one_clip("loudness", x)], [sr], None if channel_weights is None else [channel_weights],
                       true_peak=true_peak, loudness_range=loudness_range)
    parts = [r["rows"][0]] + ([r["true_peak"]] if true_peak else []) + \
        ([r["lra"], r["max_momentary"], r["max_short_term"], r["windows"].double()] if loudness_range else [])
    v = (torch.cat([p.reshape(-1) for p in parts]) if len(parts) > 1 else parts[0]).cpu().tolist()
    out = dict(lufs=v[0], peak=v[1], blocks=int(v[2]), blocks_abs=int(v[3]))
    if true_peak:
        out["true_peak"] = v[4]
    if loudness_range:
        lra, mom, st, n = v[-4:]
        out.update(lra=lra, max_momentary=mom, max_short_term=st, windows=int(n))
    return out
