"""The wave front door: what the reference gets from `librosa.load(path, sr=14000)`
(M1/dataset.py:226, M2/predict.py:288,297,303) and hands to `librosa.output.write_wav(path, y, sr)`
(M2/predict.py:515-528), with the same names and argument meaning:

  load(path, sr=22050, mono=True, offset=0.0, duration=None, dtype=np.float32, res_type='kaiser_best') -> (y, sr)
  resample(y, orig_sr, target_sr, res_type='kaiser_best', fix=True, scale=False)
  load_batch(paths, ...) / resample_batch(ys, ...): the same for a list of files / signals of any lengths, in a number
      of launches and copies that does not grow with the list (`load_batch_device` / `resample_batch_device` stay in HBM)
  to_mono(y)
  write_wav(path, y, sr, norm=False)
These live here; `load_device` keeps the result in HBM for the pipeline.  What they stand on, and what recordings.py needs beyond
librosa's names, keeps its name under `audio_io.` and lives one layer down:
  wave_file.py: the RIFF container and the table of sample formats, host only (read_wave, wave_info, wave_container, write_wav, ..)
  resampling.py: the Kaiser table, resample_device / resample_batch_device, band_gains_batch_device / resample_merge_batch_device
  planes.py: every channel as an f32 plane (load_channels_batch_device, decode_planes_batch_device, encode_batch_device, G.711,
      loudness_gain_batch_device, limit_batch_device) and pcm_to_mono_device, the mix-down under load
  stream_resampling.py: StreamResampler / StreamBandMerger, the resamplers for audio that is still arriving
No CPU fallback."""
import numpy as np
import torch

from . import ragged
from .planes import (DITHER, DITHER_FORMATS, LIMITER_MAX_LOOKAHEAD, LIMITER_TILE, decode_planes_batch_device, encode_batch_device, g711_decode_device, g711_encode_device,  # noqa: F401
                     limit_batch_device, limiter_lookahead, load_channels_batch_device, loudness_gain_batch_device, pcm_encode_device, pcm_to_mono_device,
                     planes_of, planes_together)
from .resampling import (KAISER_BEST, band_gains_batch_device, filter_on, resample_batch_device, resample_device,  # noqa: F401
                         resample_merge_batch_device, sinc_window)
from .stream_resampling import StreamBandMerger, StreamResampler  # noqa: F401
from .wave_file import (DECODE, ENCODINGS, G711, WaveFormatError, file_groups, read_wave, read_wave_info, wave_bytes,  # noqa: F401
                        wave_container, wave_info, write_wav)

# two private names that tests written against the one-module audio_io read, as views of their new homes
_filter_on = filter_on
_FMT = {kind: code for kind, (family, code) in DECODE.items() if family == "pcm"}


def _read_span(path, offset, duration, device):
    """The head of load_device: the file's samples cut to offset / duration -> (array, kind, native rate, the empty result for
    a span without a frame or None)."""
    arr, kind, sr_native = read_wave(path)
    if offset:
        arr = arr[int(offset * sr_native):]
    if duration is not None:
        arr = arr[:int(duration * sr_native)]
    return arr, kind, sr_native, None if arr.shape[0] else torch.zeros(0, dtype=torch.float32, device=device)


def load_device(path, sr=22050, mono=True, offset=0.0, duration=None, res_type="kaiser_best", device="cuda"):
    """`librosa.load` with the result left in HBM: (y f32 GPU tensor, sr).  mono=False is not on the
    reference's path (every call site takes the default) and raises."""
    if not mono:
        raise NotImplementedError("load(mono=False): the reference only loads mono (M1/dataset.py:226)")
    if not torch.cuda.is_available():
        raise RuntimeError("sos_amd.audio_io needs an MI355X: there is no CPU fallback")
    arr, kind, sr_native, empty = _read_span(path, offset, duration, device)
    if empty is not None:
        return empty, (sr_native if sr is None else sr)
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
    arrs, kinds, rates, ys = ([None] * len(paths) for _ in range(4))
    for i, path in enumerate(paths):
        arrs[i], kinds[i], rates[i], ys[i] = _read_span(path, offset, duration, device)
    by_format = ragged.group_by([(k, a.shape[1]) for k, a in zip(kinds, arrs)], lambda i, _: ys[i] is not None)
    for (kind, _), idx in by_format.items():
        pcm = torch.from_numpy(np.concatenate([arrs[i] for i in idx])).to(device)
        mono_all = pcm_to_mono_device(pcm, kind)          # per frame: the concatenation needs no table
        for i, y in zip(idx, ragged.split(mono_all, [arrs[i].shape[0] for i in idx])):
            ys[i] = y
    if sr is None:
        return ys, rates
    ys = ragged.per_group(ys, rates, lambda r, idx: resample_batch_device([ys[i] for i in idx], r, sr, res_type),
                          lambda i, r: r == sr or not ys[i].numel())
    return ys, [sr] * len(paths)


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
