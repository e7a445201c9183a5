"""Ground-truth silent-interval labels of clean speech: the `bit_stream` (one character per video frame, '0' = silent) that a
data-set JSON carries for training (`dataset.get_dataloader(dataset_json=...)`) and scoring (`handoff.detect_files`), computed
on the GPU for ragged batches of clips (csrc/silence_label.hip), and the data-set JSON itself for a list of WAVE files.

The rule is this project's own: the reference's preprocessing/ (ffmpeg, pytube and its labeller get_bitstream_better) is out of
scope and its source is not available, so parity with get_bitstream_better is unpinned.  The contract,
restated in float64 by tests/silence_reference.py, per clip of n samples at `sr` with `fps` video frames per second:

  frames   F = ceil(n fps / sr); frame i = samples [int(i r), min(int((i+1) r), n)), r = sr / fps in double (> 1).  Where the
           rounding of those products would leave the last frame empty or a sample over, F moves by one (`frame_count`).
  energy   E[i] = mean of x^2 over frame i, float64.
  raw      quiet[i] = E[i] <= T,  T = max(10^(-threshold_db / 10) max E, floor): an all-zero clip is all quiet.
  pass 1   a run of non-quiet frames shorter than min_speech with quiet frames on both sides turns quiet.
  pass 2   of the runs as pass 1 left them, a run of quiet frames shorter than min_silence turns non-quiet, wherever it lies.

min_silence / min_speech are seconds, max(1, int(round(seconds fps))) frames per clip; one frame disables a pass.  The bits are
1 = non-silent, the convention of `tools.bits_to_mask_batch`.  A batch goes up once and is labelled by one launch sequence per
65535 clips with one wait; a clip's bits and energies depend on that clip alone.  Clips: 1-D numpy arrays or GPU tensors.  No
CPU fallback."""
import json
import math
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib as L
from . import ragged

_OUT = 6                            # f64 per clip of sos_silence_label_batch: max E, T, silent frames, silent runs, frames, status
DEFAULT_MAX_BYTES = 1 << 30         # label_files: f32 samples per group of files

# What one launch sequence leaves on the device.  flat: the clips back to back (f32, plus one sentinel sample); table: host int64
# rows {sample offset, samples, frame offset, frames}; bits: uint8, 1 = non-silent, back to back at the frame offsets; ratios:
# host f64 samples per frame.  `tools.ragged_stage(flat, table, stride, bits, ratios)` takes them as they are.  energy: f64 per
# frame like bits; summary: f64 [clips][6] = {max E, T, silent frames, silent runs, frames, status}.
LabelBatch = namedtuple("LabelBatch", "flat table bits ratios energy summary")


def frame_count(n, sr, fps):
    """Frames of a clip of n samples at `sr` for video at `fps`: ceil(n fps / sr), moved until
    int((F-1) r) < n <= int(F r), r = sr / fps -- every frame holds a sample and no sample is left over (the two differ only
    where the double products round across an integer)."""
    ratio = sr / fps
    F = max(1, int(math.ceil(n * fps / sr)))
    while int(F * ratio) < n:
        F += 1
    while F > 1 and int((F - 1) * ratio) >= n:
        F -= 1
    return F


def _plan(lens, sr, fps, threshold_db, min_silence, min_speech, floor, first_clip=0):
    """Host table int64 [B][4] and parameters f64 [B][5] of sos_silence_label_batch for clips of `lens` samples."""
    par, frames = np.zeros((len(lens), 5), dtype=np.float64), []
    rel = float(10.0 ** (-float(threshold_db) / 10.0))
    if not rel >= 0.0 or not float(floor) >= 0.0:
        raise ValueError(f"threshold_db {threshold_db!r} / floor {floor!r}: the threshold must not be negative")
    if min_silence < 0 or min_speech < 0:
        raise ValueError("min_silence and min_speech are non-negative seconds")
    for b, n in enumerate(lens):
        n, s, f = int(n), float(sr[b]), float(fps[b])
        if n < 1:
            raise ValueError(f"clip {first_clip + b} is empty")
        if not (s > 0 and f > 0) or not s / f > 1.0:
            raise ValueError(f"clip {first_clip + b}: sample rate {s!r} and frame rate {f!r} must be positive with more than one "
                             "sample per frame")
        frames.append(frame_count(n, s, f))
        par[b] = (s / f, rel, float(floor), max(1, int(round(min_silence * f))), max(1, int(round(min_speech * f))))
    return ragged.clip_table(lens, frames), par


_Staged = namedtuple("_Staged", "flat tab par d_tab d_par ws bits energy summary")


def _stage(clips, sr, fps, threshold_db, min_silence, min_speech, floor, first_clip=0):
    """One launch sequence's worth of clips on the device: the concatenated samples, the table and the parameters (host and
    device), the workspace and the result buffers."""
    from .engine import upload
    for i, c in enumerate(clips):
        if int(np.prod(np.shape(c))) == 0:
            raise ValueError(f"clip {first_clip + i} is empty")
    flat, lens = ragged.concat(clips)
    tab, par = _plan(lens, sr, fps, threshold_db, min_silence, min_speech, floor, first_clip)
    B, dev = len(lens), flat.device
    nbytes = L.lib().sos_silence_label_workspace_bytes(tab.ctypes.data, B)
    if nbytes < 0:
        L.check(-22, "sos_silence_label_workspace_bytes")
    ftot = int(tab[:, 3].sum())
    return _Staged(flat, tab, par, upload(tab, torch.int64, dev), upload(par, torch.float64, dev),
                   torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev),
                   torch.empty(ftot, dtype=torch.uint8, device=dev), torch.empty(ftot, dtype=torch.float64, device=dev),
                   torch.empty((B, _OUT), dtype=torch.float64, device=dev))


def _launch(st):
    """Enqueue sos_silence_label_batch on staged clips; no wait.  -> LabelBatch."""
    L.check(L.lib().sos_silence_label_batch(L.ptr(st.flat), L.ptr(st.d_tab), st.tab.ctypes.data, len(st.tab), L.ptr(st.d_par),
                                            st.par.ctypes.data, L.ptr(st.ws), st.ws.numel(), L.ptr(st.bits), L.ptr(st.energy),
                                            L.ptr(st.summary), L.stream_ptr()), "sos_silence_label_batch")
    return LabelBatch(st.flat, st.tab, st.bits, st.par[:, 0].copy(), st.energy, st.summary)


def _enqueue(clips, sr, fps, threshold_db, min_silence, min_speech, floor, first_clip=0):
    return _launch(_stage(clips, sr, fps, threshold_db, min_silence, min_speech, floor, first_clip))


def _check_summary(rows, tab, first_clip=0):
    bad = np.flatnonzero((rows[:, 5] < 0) | (rows[:, 4] != tab[:, 3]))
    if len(bad):
        raise RuntimeError(f"sos_silence_label_batch: clip {first_clip + int(bad[0])}: the device table disagrees with the host's")


def silence_bits_batch_device(clips, sr, fps=30.0, threshold_db=40.0, min_silence=0.1, min_speech=0.0, floor=0.0):
    """silence_bits_batch with everything left on the device: a LabelBatch (at most 65535 clips; nothing is downloaded and
    nothing waited for, so `summary` has not been checked).  `tools.ragged_stage(lb.flat, lb.table, stride, lb.bits, lb.ratios)`
    stages the labelled clips for the networks."""
    clips = list(clips)
    if not 1 <= len(clips) <= ragged.MAX_CLIPS:
        raise ValueError(f"1 .. {ragged.MAX_CLIPS} clips per launch sequence, got {len(clips)}")
    return _enqueue(clips, ragged.per_clip(sr, len(clips), "sr"), ragged.per_clip(fps, len(clips), "fps"), threshold_db,
                    min_silence, min_speech, floor)


def silence_bits_batch(clips, sr, fps=30.0, threshold_db=40.0, min_silence=0.1, min_speech=0.0, floor=0.0, return_detail=False):
    """The silent-interval labels of every clip (1-D numpy arrays or GPU tensors of any lengths) sampled at `sr` for video at
    `fps` frames per second (each a scalar or one value per clip): a list of np.uint8 arrays, one value per video frame,
    1 = non-silent, 0 = silent (the module docstring states the rule; parity with the reference's labeller is unpinned).
    return_detail=True returns (bits, detail) with per clip dict(energy f64 per frame, max_energy, threshold, silent_frames,
    silent_runs).  One upload, one launch sequence per 65535 clips, one wait.  An empty clip, a non-positive rate or
    sr / fps <= 1 raises ValueError naming the clip."""
    clips = list(clips)
    B = len(clips)
    sr, fps = ragged.per_clip(sr, B, "sr"), ragged.per_clip(fps, B, "fps")
    done = []
    for c0 in range(0, B, ragged.MAX_CLIPS):
        c1 = min(B, c0 + ragged.MAX_CLIPS)
        done.append(_enqueue(clips[c0:c1], sr[c0:c1], fps[c0:c1], threshold_db, min_silence, min_speech, floor, c0))
    bits, detail = [], []
    if not done:
        return (bits, detail) if return_detail else bits
    # one copy: every chunk's f64 arrays first (energies, then the summary rows), every chunk's bits after them
    parts = [t for lb in done for t in (lb.energy.view(torch.uint8), lb.summary.reshape(-1).view(torch.uint8))]
    buf = torch.cat(parts + [lb.bits for lb in done]).cpu().numpy()      # the one wait of the call
    pos, bpos, first = 0, sum(p.numel() for p in parts), 0
    for lb in done:
        nb, ftot = len(lb.table), lb.bits.numel()
        energy = np.frombuffer(buf, np.float64, ftot, pos)
        rows = np.frombuffer(buf, np.float64, _OUT * nb, pos + 8 * ftot).reshape(nb, _OUT)
        b8 = np.frombuffer(buf, np.uint8, ftot, bpos)
        pos += 8 * ftot + 8 * _OUT * nb
        bpos += ftot
        _check_summary(rows, lb.table, first)
        for b in range(nb):
            f0, F = int(lb.table[b, 2]), int(lb.table[b, 3])
            bits.append(b8[f0:f0 + F].copy())
            if return_detail:
                detail.append(dict(energy=energy[f0:f0 + F].copy(), max_energy=float(rows[b, 0]), threshold=float(rows[b, 1]),
                                   silent_frames=int(rows[b, 2]), silent_runs=int(rows[b, 3])))
        first += nb
    return (bits, detail) if return_detail else bits


def silence_bits(clip, sr, fps=30.0, threshold_db=40.0, min_silence=0.1, min_speech=0.0, floor=0.0, return_detail=False):
    """silence_bits_batch of one clip."""
    res = silence_bits_batch([clip], sr, fps, threshold_db, min_silence, min_speech, floor, return_detail)
    return (res[0][0], res[1][0]) if return_detail else res[0]


def _plain(v):
    """30.0 -> 30, as the reference's JSON writes whole rates."""
    return int(v) if float(v) == int(v) else float(v)


def label_files(paths, output_json=None, dataset_path=None, fps=30.0, threshold_db=40.0, min_silence=0.1, min_speech=0.0,
                floor=0.0, max_bytes=DEFAULT_MAX_BYTES):
    """The data-set JSON (PP/tools.py:28-31; the keys and their order of the reference's files) of a list of clean-speech WAVE
    files, labelled with silence_bits_batch at their native sample rates: dict(dataset_path, num_videos, files), every file with
    path, clip_start_time 0, clip_end_time, face_x 0, face_y 0, framerate, audio_sample_rate, audio_samples, duration
    (round(n / sr, 2)), num_frames, bit_stream ('0' = silent), silence_total_ratio (silent frames / frames),
    avg_silenceInterval_silcenceTotal_ratio (mean silent-run length / silent frames, 0 without silence), frames_path None,
    flows_path None, audio_path.  Files are read with audio_io.load_batch_device(paths, sr=None) in groups of at most `max_bytes`
    of samples, one launch sequence and one download per group.  dataset_path defaults to the files' common directory;
    output_json: also written there with handoff.JSON_DUMP_PARAMS.  What `get_dataloader(dataset_json=...)` and
    `handoff.detect_files` read.  The labels are this project's rule: parity with the reference's labeller is unpinned."""
    from . import audio_io
    from .handoff import JSON_DUMP_PARAMS
    paths = [os.path.abspath(p) for p in paths]
    files = []
    for group in audio_io.file_groups(paths, max_bytes):
        ys, srs = audio_io.load_batch_device([paths[i] for i in group], sr=None)
        for i, y in zip(group, ys):
            if y.numel() == 0:
                raise ValueError(f"{paths[i]}: no samples")
        bits, detail = silence_bits_batch(ys, srs, fps, threshold_db, min_silence, min_speech, floor, return_detail=True)
        for i, y, sr, b, d in zip(group, ys, srs, bits, detail):
            n, F, silent, runs = y.numel(), len(b), d["silent_frames"], d["silent_runs"]
            duration = round(n / sr, 2)
            files.append(OrderedDict([
                ("path", paths[i]), ("clip_start_time", 0), ("clip_end_time", duration), ("face_x", 0), ("face_y", 0),
                ("framerate", _plain(fps)), ("audio_sample_rate", _plain(sr)), ("audio_samples", n), ("duration", duration),
                ("num_frames", F), ("bit_stream", "".join("1" if v else "0" for v in b)),
                ("silence_total_ratio", silent / F if silent else 0),
                ("avg_silenceInterval_silcenceTotal_ratio", (silent / runs) / silent if silent else 0),
                ("frames_path", None), ("flows_path", None), ("audio_path", paths[i])]))
    if dataset_path is None:
        dataset_path = os.path.commonpath([os.path.dirname(p) for p in paths]) if paths else ""
    out = OrderedDict([("dataset_path", dataset_path), ("num_videos", len(files)), ("files", files)])
    if output_json is not None:
        with open(output_json, "w") as fp:
            json.dump(out, fp, **JSON_DUMP_PARAMS)
    return out
