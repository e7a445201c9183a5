"""The on-disk hand-off between the two models, so the build interoperates stage by stage
with the reference's scripts on the README's real-recording path (`--unknown_clean_signal true`):

  dataset JSON (PP/tools.py:28-31; data/sounds_of_silence.json)
    -> detect_files                 M1/predict.py:38-233  `evaluate(clean_audio=False)`   -> eval_results.json
    -> create_data_from_prediction  M1/create_data_from_pred.py:38-271 (clean_audio=False) -> pred_data.json + recovered/*_mixed.wav
    -> get_data_from_first_model    M2/predict.py:255-374 (unknown_clean_signal=True)
    -> denoise_files                M2/predict.py:377-576                                  -> <id>/{noisy_input,noise_intervals,
                                                                     predicted_full_noise,denoised_output}.wav, stat.json, eval_results.json

Same keys, key order, value types and JSON formatting as the reference writes (checked against the reference's
own checked-in outputs in tests/golden/handoff/).  Both branches of the scripts are covered: real recordings
(`--unknown_clean_signal true`) and clean recordings mixed with noise at an SNR (clean_audio=True: noise bookkeeping,
`_mixed / _clean / _full_noise` WAVE files, objective measures in stat.json).  The PNG plots (cv2 / matplotlib) are
not built; the `waveform` / `spectrum` keys are therefore absent from stat.json.  All signal work (decode, resample,
STFT, networks, masks, ISTFT, measures) runs on the GPU through audio_io / transform / tools / metrics; this module is
the host-side bookkeeping around it."""
import json
import os
from collections import OrderedDict
from itertools import groupby
from operator import itemgetter

import numpy as np
import torch

from . import audio_io, metrics, ragged, tools, transform
from .tools import add_signals

JSON_DUMP_PARAMS = dict(indent=4, sort_keys=False, ensure_ascii=False, separators=(',', ':'))   # M1/tools.py:36
BITSTREAM_JSON_LABEL = 'bit_stream'            # M1/tools.py:54
BIT_STREAM_LABEL = 'recovered_prediction'      # M2/predict.py:30
GT_BIT_STREAM_LABEL = 'bit_stream'             # M2/predict.py:32
CLIP_FRAMES = 60                               # M1/dataset.py:33
SILENT_CONSECUTIVE_FRAMES = 1                  # M1/dataset.py:32
SIGMOID_THRESHOLD = 0.5                        # M1/predict.py:30
DATA_REQUIRED_SR = 14000                       # M1/dataset.py:38


def ensure_dir(path):
    os.makedirs(path, exist_ok=True)


def get_parent_dir(path):
    return os.path.abspath(os.path.join(path, os.pardir))


def find_common_path(str1, str2, sep='/'):
    """M1/utils.py:189-191."""
    return os.path.commonprefix([str1, str2]).rpartition(sep)[0]


def convert_snr_to_suffix2(snr):
    """M1/tools.py:882-891: None -> '', 10.0 -> '_snr10', 2.5 -> '_snr2_5'."""
    if snr is None:
        return ""
    try:
        snr = float(snr)
    except (TypeError, ValueError):
        return ""
    return '_snr' + str(int(snr) if snr.is_integer() else snr).replace('.', '_')


def convert_threshold_to_suffix(threshold_str):
    """M1/create_data_from_pred.py:26-35."""
    try:
        threshold = float(threshold_str)
    except (TypeError, ValueError):
        return ""
    return '_' + str(threshold).replace('.', '_') if 0 <= threshold <= 1 else ""


def show_metrics(y_true, y_score):
    """M1/tools.py:91-197.  Labels: 1 = non-silent, 0 = silent; SILENT is the positive class of the
    confusion counts.  Rates whose denominator is zero come out as NaN -> JSON null (the reference divides
    numpy scalars, which yields nan rather than raising)."""
    y_true = np.asarray(y_true).astype(np.int64)
    y_score = np.asarray(y_score).astype(np.int64)
    n = len(y_true)
    n_silent = int(np.sum(y_true == 0))
    n_non_silent = int(np.sum(y_true == 1))
    base = n_non_silent / n
    accuracy = int(np.sum(y_true == y_score)) / n
    t, s = 1 - y_true, 1 - y_score
    tp = int(np.sum(t * s))
    fp = int(np.sum((t == 0) * s))
    tn = int(np.sum((t == 0) * (s == 0)))
    fn = int(np.sum(t * (s == 0)))

    def div(a, b):
        return float(a) / float(b) if b else float('nan')

    tpr = div(tp, tp + fn)
    fpr = div(fp, fp + tn)
    precision = div(tp, tp + fp)
    tnr = 1 - fpr
    f1 = div(2 * tp, 2 * tp + fp + fn)
    auc = (tpr + tnr) / 2
    den = float(np.sqrt(float(tp + fp) * float(tp + fn) * float(tn + fp) * float(tn + fn)))
    mcc = 0.0 if den == 0 else (tp * tn - fp * fn) / den

    def nan_to_null(v):
        return None if isinstance(v, float) and np.isnan(v) else v

    return OrderedDict([
        ('num_samples', n), ('num_silent_samples', n_silent), ('num_non_silent_samples', n_non_silent),
        ('base', base), ('accuracy', accuracy),
        ('true_positive', tp), ('false_positive', fp), ('true_negative', tn), ('false_negative', fn),
        ('true_pos_rate(recall)', nan_to_null(tpr)), ('false_pos_rate', nan_to_null(fpr)),
        ('precision', nan_to_null(precision)), ('true_neg_rate', nan_to_null(tnr)), ('f1', nan_to_null(f1)),
        ('roc_auc', nan_to_null(auc)), ('mcc', nan_to_null(float(mcc)))])


_trim_unknown = tools.trim_unknown_frames


def _resolve(path, dataset_path, data_root):
    """The JSONs carry the authors' absolute paths; `data_root` re-roots them onto this machine."""
    if data_root is None or not dataset_path or not path.startswith(dataset_path):
        return path
    return os.path.join(data_root, os.path.relpath(path, dataset_path))


# ------------------------------------------------------------------------------------------- model 1 -> JSON
@torch.no_grad()
def add_noise_to_audio(audio, noise, snr, start_pos=0, norm=0.5):
    """M1/tools.py:846-869 with an explicit start position: crop (zero-pad) the noise to the audio, mix at `snr` dB,
    peak-normalise to `norm` (add_signals, M1/tools.py = M2/tools.py:217-276).  numpy in, numpy out."""
    crop = np.asarray(noise)[start_pos:start_pos + len(audio)]
    if len(crop) < len(audio):
        crop = np.concatenate((crop, np.zeros(len(audio) - len(crop), dtype=crop.dtype)))
    return add_signals(np.asarray(audio), [crop], snr=snr, norm=norm)


def _detect_item(data_id, f, bits_full, i1, label, pred, conf):
    """One `data` entry of eval_results.json (M1/predict.py:150-175) from a file's host arrays of decisions and confidences."""
    pred_label = [str(int(b)) for b in pred]
    return OrderedDict([
        ('id', data_id), ('path', f['path']), ('full_bit_stream', bits_full), ('num_frames', f['num_frames']),
        ('framerate', f['framerate']), ('audio_sample_rate', f['audio_sample_rate']),
        ('audio_samples', f['audio_samples']), ('duration', f['duration']), ('frame_start_idx', i1),
        ('label', label), ('pred_label', pred_label), ('match', label == pred_label),
        ('confidence', [str(c) for c in conf])])


@torch.no_grad()
def _detect_groups(net, pending, max_batch, max_columns):
    """detect_files(batch_files=True): the (id, file, bit stream, first frame, label, 14 kHz signal) entries through the
    detector in ragged groups; the stat entries in file order.  The decisions are taken from the one array that comes down per
    group: sos_threshold_bits' confidence s, whose bit is s >= threshold in f32 -- the same comparison on the host."""
    from . import engine as E
    from . import pipeline
    clips = [p[5].contiguous() for p in pending]
    items = [None] * len(pending)
    for part in pipeline._ragged_groups(clips, max_batch, max_columns):
        wave, ns = pipeline.stage_group([clips[i] for i in part])
        nv = [len(pending[i][4]) for i in part]
        rag = E.Ragged([1 + n // transform.HOP_LENGTH for n in ns], wave.device, n_vframes=nv, n_samples=ns)
        S = transform.stft_batch(wave, clip_samples=rag.tab(ns))
        logits = net(s=S, v_num_frames=max(nv), rag=rag)
        _, conf = tools.threshold_bits(logits, SIGMOID_THRESHOLD)
        conf = conf.cpu().numpy()
        for k, i in enumerate(part):
            c = conf[k, :nv[k]]
            items[i] = _detect_item(*pending[i][:5], (c >= np.float32(SIGMOID_THRESHOLD)).astype(np.uint8), c)
    return items


@torch.no_grad()
def _detect_windows(net, pending, window_seconds, context_seconds, max_batch, max_columns):
    """detect_files(window_seconds=...): the entries of _detect_groups through pipeline.detect_long -- the recordings in
    overlapping windows, ONE stitched logit stream per file at the file's own framerate and label length -- and the same one
    thresholding launch and download of confidences for all of them."""
    from . import pipeline
    pairs = pipeline.detect_long(net, [p[5].contiguous() for p in pending], sr=DATA_REQUIRED_SR, fps=[p[1]['framerate'] for p in pending],
                                 window_seconds=window_seconds, context_seconds=context_seconds, max_batch=max_batch,
                                 max_columns=max_columns, n_frames=[len(p[4]) for p in pending])
    _, conf = tools.threshold_bits(torch.cat([lg for lg, _ in pairs]), SIGMOID_THRESHOLD)
    conf = ragged.split(conf.cpu().numpy(), [len(p[4]) for p in pending])
    return [_detect_item(*p[:5], (c >= np.float32(SIGMOID_THRESHOLD)).astype(np.uint8), c) for p, c in zip(pending, conf)]


def _mix_pending(pending, mixes, noises, snr, max_bytes):
    """detect_files(batch_mix=True): the recordings of `pending` silenced on their labelled silent intervals and mixed with
    their noise crops on the device, one tools.add_signals_ragged call per group of files of at most max_bytes of samples.
    mixes: per file (noise index, first noise sample, valid samples); noises: the decoded noise files by index."""
    used = sorted({m[0] for m in mixes})
    slot = {k: j for j, k in enumerate(used)}
    out = []
    for group in ragged.byte_groups([4 * p[5].numel() for p in pending], max_bytes):
        bits = [np.asarray([int(b) for b in pending[i][4]], dtype=np.uint8) if pending[i][4] else None for i in group]
        ratios = [float(DATA_REQUIRED_SR) / pending[i][1]['framerate'] if b is not None else None for i, b in zip(group, bits)]
        mixed, _, _ = tools.add_signals_ragged([pending[i][5] for i in group], [noises[k] for k in used], snr,
                                               noise_index=[slot[mixes[i][0]] for i in group], starts=[mixes[i][1] for i in group],
                                               counts=[mixes[i][2] for i in group], bits=bits, ratios=ratios, norm=0.5)
        out += [pending[i][:5] + (m,) for i, m in zip(group, mixed)]
    return out


def detect_files(net, dataset_json, outputs, data_root=None, save_stat=True, noise_files=None, snr=None, seed=0,
                 batch_files=False, max_batch=64, max_columns=65536, batch_mix=False, max_mix_bytes=1 << 30,
                 window_seconds=None, context_seconds=2.0):
    """Whole-file silent-interval detection of every file of a dataset JSON (`evaluate`, M1/predict.py:38-233 with
    the prediction-phase items of M1/tools.py:297-332 and M1/dataset.py:226-252): one item per file, the whole
    recording at 14 kHz -> STFT -> net(s, v_num_frames=len(bits)) -> sigmoid -> >= 0.5.  Returns the stat dict and
    writes <outputs>/eval_results<suffix>.json.
    `noise_files` + `snr` select the clean-recordings branch (clean_audio=True): the recording is silenced on its
    labelled silent intervals, a crop of a noise file is mixed in at `snr` dB (peak 0.5) before detection, and the
    crop + its bookkeeping go to <outputs>/noise_snr<snr>/ (M1/predict.py:82-104) for create_data_from_prediction.
    The reference draws noise file and crop from Python's `random` stream; here a seeded numpy generator does
    (the draws themselves are not reproducible across the two).
    batch_files=True: every recording comes from one audio_io.load_batch_device call and detection runs in ragged groups
    (files sorted by length, cut into groups of <= max_batch files and <= max_columns spectrogram columns like
    pipeline.denoise_ragged's): one staging launch, one STFT, one detector call with per-file geometry, one thresholding launch
    and one download per group.  The clean-recordings branch keeps its per-file draws and mixing in file order (a seeded run
    draws the same crops).  Same JSON as the per-file form: schema, key order, file order, sort.
    batch_mix=True (with noise_files and batch_files=True; ValueError otherwise): the draws stay per file in file order -- the
    same seeded generator, so the same noise files and JSON in noise<suffix>/ byte for byte -- but every distinct noise file is
    decoded once and the recordings are silenced and mixed on the device by one tools.add_signals_ragged call per group of
    files (groups of at most max_mix_bytes of samples); recordings and mixes never visit the host.  The mixes may differ
    from the per-file kernel's in the last bit.
    window_seconds (with batch_files=True; ValueError otherwise): recordings of any length.  The recordings (after the optional
    mixing) go through pipeline.detect_long in overlapping windows of `window_seconds` cores and `context_seconds` more on each
    inner side, at each file's own `framerate` and with as many decisions as its label holds; `confidence` and `pred_label`
    come from the stitched logits.  Memory follows max_columns, not the longest file, and the 4 GB image limit of a whole-file
    detector pass is gone.  A file shorter than two cores is one window: the same JSON as batch_files=True alone."""
    if window_seconds is not None and not batch_files:
        raise ValueError("window_seconds applies to batch_files=True")
    with open(dataset_json, 'r') as fp:
        ds = json.load(fp)
    net.eval()
    stat = []
    clean_audio = noise_files is not None
    if batch_mix and not (batch_files and clean_audio):
        raise ValueError("batch_mix=True applies to noise_files given with batch_files=True")
    if clean_audio and snr is None:
        raise ValueError("the clean-recordings branch needs an snr")
    suffix = convert_snr_to_suffix2(snr) if clean_audio else ''
    rng = np.random.default_rng(seed)
    noise_entries = OrderedDict()
    loaded, pending = None, []
    decoded, mixes = {}, []                                     # batch_mix: noise files by index, per-file crops
    if batch_files and ds['files']:
        loaded, _ = audio_io.load_batch_device([_resolve(f['audio_path'], ds.get('dataset_path'), data_root) for f in ds['files']],
                                               sr=DATA_REQUIRED_SR)
    for data_id, f in enumerate(ds['files']):
        bits_full = f[BITSTREAM_JSON_LABEL]
        i1, i2 = _trim_unknown(bits_full)
        label = [str(int(b)) for b in bits_full[i1:i2]]
        if batch_files:
            snd = loaded[data_id]
        else:
            snd, _ = audio_io.load_device(_resolve(f['audio_path'], ds.get('dataset_path'), data_root), sr=DATA_REQUIRED_SR)
        if batch_mix:
            k = int(rng.integers(len(noise_files)))
            if k not in decoded:
                decoded[k] = audio_io.load(noise_files[k], sr=DATA_REQUIRED_SR)[0]
            noise = decoded[k]
            need = int(np.ceil(f['duration'])) * DATA_REQUIRED_SR
            start = int(rng.integers(0, max(len(noise) - need, 0) + 1))
            crop = noise[start:start + need]                        # M1/dataset.py:141-142
            start_pos = int(i1 / f['framerate'] * DATA_REQUIRED_SR)
            mixes.append((k, start + start_pos, max(len(crop) - start_pos, 0)))
            base = os.path.basename(f['path'])
            noise_name = base.split('.mp4')[0].split('.wav')[0] + '_noise.wav'
            noise_dir = os.path.join(os.path.abspath(outputs), 'noise' + suffix)
            ensure_dir(noise_dir)
            audio_io.write_wav(os.path.join(noise_dir, noise_name), crop.astype(np.float32), DATA_REQUIRED_SR)
            noise_entries[base] = OrderedDict([('audio', base.split('.mp4')[0].split('.wav')[0] + '.wav'),
                                               ('noise', noise_name), ('snr', snr)])
            pending.append((data_id, f, bits_full, i1, label, snd))     # mixed after the loop, in groups
            continue
        if clean_audio:
            gt = torch.tensor([int(b) for b in label], dtype=torch.uint8, device=snd.device).reshape(1, -1)
            gmask = tools.bits_to_mask_batch(gt, float(DATA_REQUIRED_SR) / f['framerate'], snd.numel())
            audio = (snd * (1 - gmask[0])).cpu().numpy()            # M1/dataset.py:247-249
            noise, _ = audio_io.load(noise_files[int(rng.integers(len(noise_files)))], sr=DATA_REQUIRED_SR)
            need = int(np.ceil(f['duration'])) * DATA_REQUIRED_SR
            start = int(rng.integers(0, max(len(noise) - need, 0) + 1))
            crop = noise[start:start + need]                        # M1/dataset.py:141-142
            mixed, _, _ = add_noise_to_audio(audio, crop, snr, start_pos=int(i1 / f['framerate'] * DATA_REQUIRED_SR))
            snd = torch.from_numpy(np.ascontiguousarray(mixed, dtype=np.float32)).to(snd.device)
            base = os.path.basename(f['path'])
            noise_name = base.split('.mp4')[0].split('.wav')[0] + '_noise.wav'
            noise_dir = os.path.join(os.path.abspath(outputs), 'noise' + suffix)
            ensure_dir(noise_dir)
            audio_io.write_wav(os.path.join(noise_dir, noise_name), crop.astype(np.float32), DATA_REQUIRED_SR)
            noise_entries[base] = OrderedDict([('audio', base.split('.mp4')[0].split('.wav')[0] + '.wav'),
                                               ('noise', noise_name), ('snr', snr)])
        if batch_files:
            pending.append((data_id, f, bits_full, i1, label, snd))
            continue
        S = transform.stft_batch(snd.reshape(1, -1))
        logits = net(s=S, v_num_frames=len(label))
        pred, conf = tools.threshold_bits(logits, SIGMOID_THRESHOLD)
        stat.append(_detect_item(data_id, f, bits_full, i1, label, pred[0].cpu().numpy(), conf[0].cpu().numpy()))
    if pending and batch_mix:
        pending = _mix_pending(pending, mixes, decoded, snr, max_mix_bytes)
    if pending:
        stat = (_detect_groups(net, pending, max_batch, max_columns) if window_seconds is None else
                _detect_windows(net, pending, window_seconds, context_seconds, max_batch, max_columns))
    stat_dict = OrderedDict([
        ('data_total_frames', CLIP_FRAMES), ('data_center_frames', SILENT_CONSECUTIVE_FRAMES),
        ('sigmoid_threshold', SIGMOID_THRESHOLD), ('snr', snr if clean_audio else None),
        ('prediction_statistics', OrderedDict([('all', show_metrics([b for it in stat for b in it['label']],
                                                                    [b for it in stat for b in it['pred_label']]))]))])
    stat_dict['data'] = sorted(stat, key=lambda x: np.mean([float(c) for c in x['confidence']]), reverse=True)
    if clean_audio:
        with open(os.path.join(os.path.abspath(outputs), 'noise' + suffix, suffix[1:] + '.json'), 'w') as fp:
            json.dump(OrderedDict([('snrs', [snr]), ('files', noise_entries)]), fp, **JSON_DUMP_PARAMS)
    if save_stat:
        ensure_dir(os.path.abspath(outputs))
        with open(os.path.join(os.path.abspath(outputs), 'eval_results' + suffix + '.json'), 'w') as fp:
            json.dump(stat_dict, fp, **JSON_DUMP_PARAMS)
    return stat_dict


def _write_recovered_batch(jobs, clean_audio, noise_dir, nsuffix, max_bytes):
    """create_data_from_prediction(batch_files=True): the WAVE files of `jobs` = (item, recording path, save_dir, name), per
    group of files one audio_io.load_batch_device for the recordings (and one for the stored noise crops, one
    tools.add_signals_ragged call) and one download."""
    from .labels import _file_groups
    noise_files = None
    if clean_audio and jobs:
        with open(os.path.join(noise_dir, nsuffix[1:] + '.json'), 'r') as fpn:
            noise_files = json.load(fpn)['files']
    for group in _file_groups([j[1] for j in jobs], max_bytes):
        part = [jobs[i] for i in group]
        snds, _ = audio_io.load_batch_device([j[1] for j in part], sr=DATA_REQUIRED_SR)
        if clean_audio:
            entries = [noise_files[os.path.basename(j[0]['path'])] for j in part]
            noises, _ = audio_io.load_batch_device([os.path.join(noise_dir, e['noise']) for e in entries], sr=DATA_REQUIRED_SR)
            mixed, clean, full_noise = tools.add_signals_ragged(snds, noises, [e['snr'] for e in entries], starts=0, norm=0.5)
            host = ragged.download(mixed + clean + full_noise, np.float32)
        else:
            host = ragged.download(snds, np.float32)
        B = len(part)
        for k, (item, _, save_dir, filename) in enumerate(part):
            mixed_path = os.path.join(save_dir, filename + '_mixed.wav')
            rel = lambda q: os.path.join(os.path.basename(save_dir), os.path.basename(q))     # noqa: E731
            audio_io.write_wav(mixed_path, host[k], DATA_REQUIRED_SR)
            if clean_audio:
                clean_path = os.path.join(save_dir, filename + '_clean.wav')
                full_noise_path = os.path.join(save_dir, filename + '_full_noise.wav')
                audio_io.write_wav(clean_path, host[B + k], DATA_REQUIRED_SR)
                audio_io.write_wav(full_noise_path, host[2 * B + k], DATA_REQUIRED_SR)
                item['mixed_audio'], item['clean_audio'], item['full_noise'] = rel(mixed_path), rel(clean_path), rel(full_noise_path)
                item['audio_path'] = clean_path
            else:
                item['mixed_audio'] = rel(mixed_path)


def create_data_from_prediction(input_json, output_json=None, suffix="", noise_snr=None, save_results=True,
                                data_root=None, clean_audio=False, batch_files=False, max_bytes=1 << 30):
    """eval_results.json -> pred_data.json (`create_data_from_prediction_newtarget_bceloss_no_voting`,
    M1/create_data_from_pred.py:38-271): per file the ground-truth, predicted and `recovered_prediction` bit
    streams; with save_results the 14 kHz signal is written to recovered<suffix>/<name>_mixed.wav next to the JSON and
    referenced as `mixed_audio`.  clean_audio=True (:158-190): the recording is mixed with the noise crop that
    detect_files stored (noise<nsuffix>/<nsuffix[1:]>.json) at its SNR, and `<name>_mixed / _clean / _full_noise.wav`
    are written and referenced (`mixed_audio`, `clean_audio`, `full_noise`, `audio_path`).
    batch_files=True (with save_results): the recordings come from one audio_io.load_batch_device call per group of files of at
    most max_bytes of samples; with clean_audio so do the stored noise crops, one tools.add_signals_ragged call mixes the group
    and its three signals per file come down in one copy.  The same WAVE files per item and the same JSON."""
    suffix = suffix or ""
    if output_json is None:
        output_json = os.path.join(get_parent_dir(input_json), 'pred_data.json')
        if suffix:
            output_json = output_json.split('.json')[0] + '{}.json'.format(suffix)
    nsuffix = convert_snr_to_suffix2(noise_snr)
    output_json = output_json.split('.json')[0] + '{}.json'.format(nsuffix)
    with open(input_json, 'r') as fp:
        obj = json.load(fp)
    items = sorted(obj['data'], key=itemgetter('id'))
    groups = []
    for path, g in groupby(items, itemgetter('path')):
        g = list(g)
        groups.append(OrderedDict([
            ('path', path), ('num_frames', g[0]['num_frames']), ('framerate', g[0]['framerate']),
            ('audio_sample_rate', g[0]['audio_sample_rate']), ('audio_samples', g[0]['audio_samples']),
            ('duration', g[0]['duration']), ('bit_stream', g[0]['full_bit_stream']),
            ('ground_truth_bit_stream', ''.join(str(int(b)) for it in g for b in it['label'])),
            ('predicted_bit_stream', ''.join(str(int(b)) for it in g for b in it['pred_label'])),
            ('recovered_prediction', None), ('overlay_original', None), ('overlay_predicted', None)]))
    ds_path, labels, pred_labels, jobs = '', [], [], []
    # the JSON carries the authors' absolute paths: `data_root` stands in for their common directory
    src_root = os.path.commonpath([os.path.dirname(g['path']) for g in groups]) if groups else ''
    for item in groups:
        ds_path = item['path'] if ds_path == '' else find_common_path(ds_path, item['path'])
        item['num_frames'] = len(item['bit_stream'])
        item['recovered_prediction'] = item['predicted_bit_stream']
        labels += [int(s) for s in item['bit_stream']]
        pred_labels += [int(s) for s in item['recovered_prediction']]
        if save_results:
            save_dir = os.path.join(get_parent_dir(input_json), 'recovered' + suffix + nsuffix)
            ensure_dir(save_dir)
            parts = item['path'].split('.mp4')
            wav_path = parts[0] if len(parts) == 1 else parts[0] + '.wav'
            if batch_files:
                jobs.append((item, _resolve(wav_path, src_root, data_root), save_dir, os.path.basename(wav_path).split('.wav')[0]))
                continue
            snd, _ = audio_io.load(_resolve(wav_path, src_root, data_root), sr=DATA_REQUIRED_SR)
            filename = os.path.basename(wav_path).split('.wav')[0]
            mixed_path = os.path.join(save_dir, filename + '_mixed.wav')
            rel = lambda q: os.path.join(os.path.basename(save_dir), os.path.basename(q))     # noqa: E731
            if clean_audio:
                noise_dir = os.path.join(get_parent_dir(output_json), 'noise' + nsuffix)
                with open(os.path.join(noise_dir, nsuffix[1:] + '.json'), 'r') as fpn:
                    noise_files = json.load(fpn)['files']
                entry = noise_files[os.path.basename(item['path'])]
                noise, _ = audio_io.load(os.path.join(noise_dir, entry['noise']), sr=DATA_REQUIRED_SR)
                mixed, clean, full_noise = add_noise_to_audio(snd, noise, entry['snr'], start_pos=0, norm=0.5)
                clean_path = os.path.join(save_dir, filename + '_clean.wav')
                full_noise_path = os.path.join(save_dir, filename + '_full_noise.wav')
                audio_io.write_wav(mixed_path, mixed.astype(np.float32), DATA_REQUIRED_SR)
                audio_io.write_wav(clean_path, clean.astype(np.float32), DATA_REQUIRED_SR)
                audio_io.write_wav(full_noise_path, full_noise[0].astype(np.float32), DATA_REQUIRED_SR)
                item['mixed_audio'], item['clean_audio'], item['full_noise'] = rel(mixed_path), rel(clean_path), rel(full_noise_path)
                item['audio_path'] = clean_path
            else:
                audio_io.write_wav(mixed_path, snd, DATA_REQUIRED_SR)
                item['mixed_audio'] = rel(mixed_path)
    if jobs:
        _write_recovered_batch(jobs, clean_audio, os.path.join(get_parent_dir(output_json), 'noise' + nsuffix), nsuffix, max_bytes)
    hierarchy = OrderedDict([
        ('dataset_path', ds_path), ('num_videos', len(groups)), ('data_total_frames', obj['data_total_frames']),
        ('data_center_frames', obj['data_center_frames']), ('sigmoid_threshold', obj['sigmoid_threshold']),
        ('snr', noise_snr), ('prediction_statistics', show_metrics(labels, pred_labels)), ('files', groups)])
    with open(output_json, 'wb') as fp:
        fp.write(json.dumps(hierarchy, **JSON_DUMP_PARAMS).encode())
    return output_json


# ------------------------------------------------------------------------------------------- JSON -> model 2
def _parse_bits(bitstream):
    """M2/predict.py:232-252: '0' / '1' (a '2' is tolerated as non-silent) -> 0 / 1 values; anything else is an error."""
    vals = []
    for bit in bitstream:
        if bit not in '012':
            print('Invalid bit?')
            raise RuntimeError
        vals.append(0 if bit == '0' else 1)
    return vals


def get_data_from_first_model(first_model_json_path, sr=DATA_REQUIRED_SR, snr=None, n_fft=510, hop_length=158,
                              win_length=400, unknown_clean_signal=True):
    """M2/predict.py:255-374: per file of pred_data.json load `mixed_audio`, turn `recovered_prediction` into the
    sample mask, noise_sig = mixed * mask, STFT both.  With unknown_clean_signal=False the file entries also name
    `clean_audio` and `full_noise` (written by the reference's create_data_from_pred.py with clean_audio=True): the
    clean signal is silenced on the ground-truth silent intervals (:321) and both are transformed too.
    Tensors stay in HBM: item['mixed'] / item['noise'] (/ 'clean' / 'full_noise') are (1, 2, 256, T) GPU tensors,
    item['mask'] a (n_samples,) GPU tensor."""
    with open(first_model_json_path, 'r') as fp:
        obj = json.load(fp)
    snr = obj['snr']
    data_list = []
    for data in obj['files']:
        mixed_audio_path = os.path.join(get_parent_dir(first_model_json_path), data['mixed_audio'])
        mixed_sig, _ = audio_io.load_device(mixed_audio_path, sr=sr)
        bitstream = data[BIT_STREAM_LABEL]
        bits = torch.tensor(_parse_bits(bitstream), dtype=torch.uint8, device=mixed_sig.device).reshape(1, -1)
        mask, noise_sig = tools.bits_to_mask_batch(bits, float(sr) / data['framerate'], mixed_sig.numel(),
                                                   mixed_sig.reshape(1, -1))
        item = OrderedDict([('id', os.path.splitext(os.path.basename(data['path']))[0]), ('path', data['path'])])
        known = OrderedDict()
        if not unknown_clean_signal:
            clean_audio_path = os.path.join(get_parent_dir(first_model_json_path), data['clean_audio'])
            full_noise_path = os.path.join(get_parent_dir(first_model_json_path), data['full_noise'])
            clean_sig, _ = audio_io.load_device(clean_audio_path, sr=sr)
            full_noise, _ = audio_io.load_device(full_noise_path, sr=sr)
            gt = torch.tensor([0 if b == '0' else 1 for b in data[GT_BIT_STREAM_LABEL]], dtype=torch.uint8,
                              device=clean_sig.device).reshape(1, -1)
            gt_mask = tools.bits_to_mask_batch(gt, float(sr) / data['framerate'], clean_sig.numel())
            clean_sig = clean_sig * (1 - gt_mask[0])             # silent intervals truly silent (M2/predict.py:321)
            item['clean_audio_path'] = clean_audio_path
            known['clean'] = transform.stft_batch(clean_sig.reshape(1, -1), n_fft, hop_length, win_length)
            known['full_noise'] = transform.stft_batch(full_noise.reshape(1, -1), n_fft, hop_length, win_length)
        item['mixed_audio_path'] = mixed_audio_path
        if not unknown_clean_signal:
            item['full_noise_path'] = full_noise_path
        item['bitstream'] = bitstream
        item['mixed'] = transform.stft_batch(mixed_sig.reshape(1, -1), n_fft, hop_length, win_length)
        if 'clean' in known:
            item['clean'] = known['clean']
        item['noise'] = transform.stft_batch(noise_sig, n_fft, hop_length, win_length)
        if 'full_noise' in known:
            item['full_noise'] = known['full_noise']
        item.update([('mask', mask[0]), ('snr', snr), ('sr', sr)])
        data_list.append(item)
    info = OrderedDict([(k, obj[k]) for k in ('dataset_path', 'num_videos', 'data_total_frames', 'data_center_frames',
                                              'sigmoid_threshold')])
    return data_list, info


def _write_individual(data, info, sigs, gt_sigs, outputs, snr, save_individual_results):
    """The WAVE files and stat.json of one file of denoise_files (M2/predict.py:515-560); fills the path keys of `info`."""
    if not save_individual_results:
        return
    _write_individual_host(data, info, sigs.cpu().numpy(), None if gt_sigs is None else gt_sigs.cpu().numpy(), outputs, snr)


def _write_individual_host(data, info, host, gh, outputs, snr):
    """_write_individual on host arrays: host (4, n) = the four signals, gh (2, >= n) = the ground-truth ones or None."""
    save_dir = os.path.join(os.path.abspath(outputs), convert_snr_to_suffix2(snr)[1:], str(data['id']))
    ensure_dir(save_dir)
    for k, name in enumerate(('noisy_input', 'noise_intervals', 'predicted_full_noise', 'denoised_output')):
        p = os.path.join(save_dir, name + '.wav')
        audio_io.write_wav(p, host[k], data['sr'])
        info[name] = p
    if gh is not None:
        for k, name in enumerate(('ground_truth_full_noise', 'ground_truth_clean_input')):
            p = os.path.join(save_dir, name + '.wav')
            audio_io.write_wav(p, gh[k][:len(host[0])], data['sr'])
            info[name] = p
    with open(os.path.join(save_dir, 'stat.json'), 'w') as fp:
        json.dump(info, fp, **JSON_DUMP_PARAMS)


def _batch_measures(work, pesq_fn, stoi_fn):
    """The objective measures of all files with a known clean signal (denoise_files(batch_metrics=True)): outputs and clean
    signals to 16 kHz in one resample_batch_device call per distinct rate (2 F clips), one evaluate_metrics_batch."""
    if not work:
        return
    out16, clean16 = [None] * len(work), [None] * len(work)
    by_rate = OrderedDict()
    for i, (data, _, _, _) in enumerate(work):
        by_rate.setdefault(data['sr'], []).append(i)
    for sr, idx in by_rate.items():
        clips = [work[i][2][3].contiguous() for i in idx] + [work[i][3][1].contiguous() for i in idx]
        res = audio_io.resample_batch_device(clips, sr, 16000)
        for k, i in enumerate(idx):
            n = min(res[k].numel(), res[len(idx) + k].numel())       # evaluate_metrics compares the common prefix
            out16[i], clean16[i] = res[k][:n], res[len(idx) + k][:n]
    pesq, stoi = None, (True if stoi_fn is True else None)
    if pesq_fn is not None or callable(stoi_fn):
        host = ragged.download(out16 + clean16)                       # one download for the callables
        oh, ch = host[:len(work)], host[len(work):]
        if pesq_fn is not None:
            pesq = [pesq_fn(c, o, 16000) for c, o in zip(ch, oh)]
        if callable(stoi_fn):
            stoi = [stoi_fn(c, o, 16000) for c, o in zip(ch, oh)]
    for (_, info, _, _), m in zip(work, metrics.evaluate_metrics_batch(out16, clean16, sr=16000, pesq=pesq, stoi=stoi)):
        info.update(m)


def _write_eval_results(data_info, stat, outputs, threshold, snr):
    """eval_results<suffixes>.json of denoise_files (M2/predict.py:562-576): the averages of the available measures and the files."""
    if stat and 'l1' in stat[0]:
        keys = ('l1', 'stoi', 'csig', 'cbak', 'covl', 'pesq', 'ssnr_regular', 'ssnr_shift', 'ssnr_clip', 'ssnr_exsi', 'overall_snr')
        data_info['denoise_statistics'] = OrderedDict(
            ('avg_' + k, (sum(it[k] for it in stat) / len(stat)) if all(it[k] is not None for it in stat) else None)
            for k in keys)
    data_info['files'] = stat
    ensure_dir(os.path.abspath(outputs))
    path = os.path.join(os.path.abspath(outputs), 'eval_results' + convert_threshold_to_suffix(threshold) +
                        convert_snr_to_suffix2(snr) + '.json')
    with open(path, 'w') as fp:
        json.dump(data_info, fp, **JSON_DUMP_PARAMS)


@torch.no_grad()
def denoise_files(net, data_list_info, outputs, snr=None, threshold="", save_individual_results=True, save_stat=True,
                  pesq_fn=None, stoi_fn=None, batch_metrics=False):
    """M2/predict.py:377-576 (`evaluate`): net(mixed, noise) -> (pred_noise, mask); mask applied to the mixed
    spectrogram; ISTFT of mixed / noise intervals / predicted noise / output written as
    <outputs>/<snr suffix>/<id>/*.wav + stat.json, and <outputs>/eval_results<suffixes>.json.  Items that carry a
    `clean` spectrogram (unknown_clean_signal=False) also get the objective measures of the output resampled to
    16 kHz against the clean signal (:455-460) and the ground-truth WAVE files; `pesq_fn(clean, output, sr)` /
    `stoi_fn(clean, output, sr)` supply the two third-party scores (None entries otherwise) and the averages of the
    available measures go to `denoise_statistics`.  `stoi_fn=metrics.stoi` computes STOI in HIP (pypesq has no
    counterpart here).
    batch_metrics=True: no file waits for the device inside the loop; afterwards the outputs and clean signals of all files
    with a known clean signal go to 16 kHz in one audio_io.resample_batch_device call per distinct rate and through one
    metrics.evaluate_metrics_batch, and the files are written after that.  `stoi_fn=True` then means STOI by
    metrics.stoi_batch in the same launch sequence; a callable `stoi_fn` / `pesq_fn` is called per clip on host arrays
    taken from one download of the resampled batch.  Same keys, order, types and files as the per-file path."""
    data_list, data_info = data_list_info
    data_info = OrderedDict(data_info)
    data_info['snr'] = snr
    net.eval()
    stat, work = [], []
    for data in data_list:
        pred_noise_stft, crm = net(data['mixed'], data['noise'])
        out_stft = transform.batch_fast_icRM_sigmoid(data['mixed'], crm)
        sigs = transform.istft_batch(torch.cat([data['mixed'], data['noise'], pred_noise_stft, out_stft], dim=0))
        known = 'clean' in data
        info = OrderedDict([('id', str(data['id'])), ('path', str(data['path']))])
        if known:
            info['clean_audio_path'] = data['clean_audio_path']
        info['mixed_audio_path'] = data['mixed_audio_path']
        if known:
            info['full_noise_path'] = data['full_noise_path']
        info.update([('bitstream', data['bitstream']), ('sr', data['sr']), ('snr', data['snr'])])
        gt_sigs = None
        if known:
            gt_sigs = transform.istft_batch(torch.cat([data['full_noise'], data['clean']], dim=0))
            if not batch_metrics:
                out16 = audio_io.resample_device(sigs[3].contiguous(), data['sr'], 16000)
                clean16 = audio_io.resample_device(gt_sigs[1].contiguous(), data['sr'], 16000)
                pesq = pesq_fn(clean16.cpu().numpy(), out16.cpu().numpy(), 16000) if pesq_fn is not None else None
                stoi = stoi_fn(clean16.cpu().numpy(), out16.cpu().numpy(), 16000) if stoi_fn is not None else None
                info.update(metrics.evaluate_metrics(out16, clean16, sr=16000, pesq=pesq, stoi=stoi))
        work.append((data, info, sigs, gt_sigs))
        if not batch_metrics:
            _write_individual(*work.pop(), outputs, snr, save_individual_results)
        stat.append(info)
    if batch_metrics:
        _batch_measures([w for w in work if w[3] is not None], pesq_fn, stoi_fn)
        for w in work:
            _write_individual(*w, outputs, snr, save_individual_results)
    if save_stat:
        _write_eval_results(data_info, stat, outputs, threshold, snr)
    return stat


def _round_trip(wave, ns):
    """STFT -> ISTFT of the rows of a padded buffer, every row at its own `ns` samples (hop * (n // hop) come back)."""
    from . import engine as E
    rag = E.Ragged([1 + n // transform.HOP_LENGTH for n in ns], wave.device, n_samples=ns)
    return transform.istft_batch(transform.stft_batch(wave, clip_samples=rag.tab(ns)), clip_frames=rag.level(0))


def _first_model_windows(net, mixed, noise, clean, all_bits, nb, ngt, ratios, framerates, sr, window_seconds, context_seconds,
                         max_batch, max_columns, download):
    """The windowed half of denoise_first_model: `mixed` (one 1-D GPU recording per file; `noise` / `clean`: the ground-truth
    recordings or empty lists), all_bits = the files' `recovered_prediction` decisions (nb each) followed by the ground-truth
    ones (ngt each) in one GPU buffer.  -> per file ([4 signals], [2 ground-truth signals] or None, host arrays of the
    4 (6) signals as _write_individual_host takes them, or None without `download`).
    The four signals: windows._masked_group(signals=True) over the windows of all files, then ONE sos_window_stitch_planes_f32 launch into
    a file-major buffer -- the four signals of a file next to each other, every segment on a multiple of four floats (16-byte
    stores) -- and ONE device-to-host copy of it, with no launch in between.
    The ground-truth signals (the STFT -> ISTFT round trips of `full_noise` and of the clean recording silenced on its
    ground-truth silent intervals) are further recordings under a plan of their own, since their lengths may differ from the
    mixed file's: sos_window_stage_f32 per group, sos_window_stage_masked_f32 and wave - masked for the clean windows
    (M2/predict.py:321), one sos_window_stitch_f32, cropped to the output length as on the whole-file path."""
    from . import windows
    F, device = len(mixed), mixed[0].device
    core, context, ns, plan = windows._long_plan("denoise_first_model", mixed, sr, window_seconds, context_seconds)
    flat, _ = ragged.concat(mixed)
    rates = np.asarray(framerates, dtype=np.float64)
    kept = windows._run_windows(plan, flat.device, max_batch, max_columns, windows._masked_group(
        net, flat, all_bits, ragged.clip_table(ns, nb), ratios, rates[plan[:, 0]], sr, signals=True), planes=4)
    lens = windows._out_lengths(ns)
    pitch = [-(-n // 4) * 4 for n in lens]
    base = (4 * ragged.offsets(pitch)).tolist()
    buf = windows._stitch_signals(kept, plan, context, recs=np.stack([base, pitch], axis=1), out_total=4 * sum(pitch))
    host = buf.cpu().numpy() if download else None              # the four signals of every file: one copy
    sigs = [[buf[base[i] + q * pitch[i]:base[i] + q * pitch[i] + lens[i]] for q in range(4)] for i in range(F)]
    hosts = [[host[base[i] + q * pitch[i]:base[i] + q * pitch[i] + lens[i]] for q in range(4)] if download else None for i in range(F)]
    if not noise:
        return sigs, [None] * F, hosts
    # recordings 0 .. F - 1: full_noise, F .. 2 F - 1: clean, with its ground-truth decisions
    _, _, ng, gplan = windows._long_plan("denoise_first_model", noise + clean, sr, window_seconds, context_seconds)
    gflat, _ = ragged.concat(noise + clean)
    gtable = ragged.clip_table(ng, [0] * F + list(ngt))
    gbits = all_bits[sum(nb):]

    def run_group(part, sub, m, rows):
        wave = tools.window_stage(gflat, sub, max(m))
        silenced = np.flatnonzero(sub[:, 0] >= F)
        if len(silenced):
            w, masked = tools.window_stage_masked(gflat, gbits, gtable, list(ratios) * 2, sub[silenced], max(m))
            wave[torch.from_numpy(silenced).to(device)] = w - masked
        return _round_trip(wave, m)

    gkept = windows._run_windows(gplan, device, max_batch, max_columns, run_group)
    gt = ragged.split(tools.window_stitch(gkept, windows._row_plan(gplan), context), windows._out_lengths(ng))
    gts = [[gt[i], gt[F + i]] for i in range(F)]
    if download:                                                 # cropped like _write_individual: one more copy
        gh = ragged.download([g[:lens[i]] for i in range(F) for g in gts[i]])
        hosts = [hosts[i] + gh[2 * i:2 * i + 2] for i in range(F)]
    return sigs, gts, hosts


@torch.no_grad()
def denoise_first_model(net, first_model_json_path, outputs, sr=DATA_REQUIRED_SR, snr=None, threshold="", unknown_clean_signal=True,
                        save_individual_results=True, save_stat=True, pesq_fn=None, stoi_fn=None, max_batch=64, max_columns=65536,
                        window_seconds=None, context_seconds=2.0):
    """get_data_from_first_model + denoise_files(batch_metrics=True) over the files of pred_data.json in ragged groups instead
    of one file at a time: the same WAVE files, stat.json, eval_results<suffixes>.json and returned `stat` list (in the JSON's
    file order), with the number of launches, copies and host waits following the number of GROUPS, not of files.
      - one audio_io.load_batch_device over every `mixed_audio` (and `clean_audio`, `full_noise` with
        unknown_clean_signal=False); the bit strings are parsed on the host and go up in one copy;
      - files sorted by length and cut into groups of <= max_batch files and <= max_columns spectrogram columns
        (pipeline._ragged_groups); a group is staged by ONE sos_ragged_stage_f32 launch -- padded recordings, noise intervals
        from `recovered_prediction` at the file's own sr / framerate, and with known clean signals the ground-truth mask of the
        clean recording in the same launch (clean * (1 - mask) is then wave - masked of its row: M2/predict.py:321) -- and runs
        as pipeline.denoise_ragged(bits=..., fps=framerates, return_all=True) runs it; the STFT -> ISTFT round trip of
        `full_noise` and the silenced clean signal are further rows of the group;
      - the four (six) signals of every file of a group come down in one copy (sos_ragged_unpack_f32);
      - the measures of all files go through _batch_measures (stoi_fn=True: STOI in the same launch sequence).
    window_seconds (None: every file runs whole, as above): files of ANY length, the counterpart of detect_files(window_seconds=).
    Every file is cut into overlapping windows (pipeline.window_plan), the windows of ALL files are grouped by max_batch /
    max_columns and staged by one sos_window_stage_masked_f32 launch per group at the file's own sr / framerate, and ONE
    sos_window_stitch_planes_f32 launch cross-fades the four signals of every file into a file-major buffer, which comes down
    in one copy (_first_model_windows).  A file shorter than two windows is one window: the whole-file computation.  Same
    files, keys, order, types and measures as the whole-file path; activation memory follows max_columns, not the file.
    A file with fewer than pipeline.MIN_FRAMES STFT frames raises ValueError naming it before any group is staged or run, and
    so do pipeline.window_plan's argument rules."""
    from . import engine as E
    from . import pipeline
    with open(first_model_json_path, 'r') as fp:
        obj = json.load(fp)
    base = get_parent_dir(first_model_json_path)
    files = obj['files']
    known = not unknown_clean_signal
    F = len(files)
    data_info = OrderedDict([(k, obj[k]) for k in ('dataset_path', 'num_videos', 'data_total_frames', 'data_center_frames',
                                                   'sigmoid_threshold')])
    data_info['snr'] = snr
    net.eval()
    mixed_paths = [os.path.join(base, d['mixed_audio']) for d in files]
    clean_paths = [os.path.join(base, d['clean_audio']) for d in files] if known else []
    noise_paths = [os.path.join(base, d['full_noise']) for d in files] if known else []
    rec_bits = [np.asarray(_parse_bits(d[BIT_STREAM_LABEL]), dtype=np.uint8) for d in files]
    gt_bits = [np.asarray([0 if b == '0' else 1 for b in d[GT_BIT_STREAM_LABEL]], dtype=np.uint8) for d in files] if known else []
    ratios = [float(sr) / d['framerate'] for d in files]
    stat, work = [], []

    def file_info(i):
        d = files[i]
        data = dict(id=os.path.splitext(os.path.basename(d['path']))[0], sr=sr)
        info = OrderedDict([('id', str(data['id'])), ('path', str(d['path']))])
        if known:
            info['clean_audio_path'] = clean_paths[i]
        info['mixed_audio_path'] = mixed_paths[i]
        if known:
            info['full_noise_path'] = noise_paths[i]
        info.update([('bitstream', d[BIT_STREAM_LABEL]), ('sr', sr), ('snr', obj['snr'])])
        return data, info

    if F:
        ys, _ = audio_io.load_batch_device(mixed_paths + clean_paths + noise_paths, sr=sr)
        mixed, clean, noise = ys[:F], ys[F:2 * F], ys[2 * F:]
        hop = transform.HOP_LENGTH
        for i, y in enumerate(mixed):
            if 1 + y.numel() // hop < pipeline.MIN_FRAMES:
                raise ValueError("%s: %d samples at %d Hz are fewer than the %d STFT frames (%d samples) the denoiser needs"
                                 % (mixed_paths[i], y.numel(), sr, pipeline.MIN_FRAMES, pipeline.MIN_FRAMES * hop))
        device = mixed[0].device
        all_bits = torch.from_numpy(np.concatenate(rec_bits + gt_bits)).to(device)       # every bit string: one copy
        d_bits = ragged.split(all_bits, [len(b) for b in rec_bits + gt_bits])
        work = [None] * F
    if F and window_seconds is not None:
        for i, y in enumerate(clean + noise):                # the ground-truth recordings are windowed under a plan of their own
            if 1 + y.numel() // hop < pipeline.MIN_FRAMES:
                raise ValueError("%s: %d samples at %d Hz are fewer than the %d STFT frames (%d samples) a window needs"
                                 % ((clean_paths + noise_paths)[i], y.numel(), sr, pipeline.MIN_FRAMES, pipeline.MIN_FRAMES * hop))
        sigs, gts, hosts = _first_model_windows(net, mixed, noise, clean, all_bits, [len(b) for b in rec_bits],
                                                [len(b) for b in gt_bits], ratios, [d['framerate'] for d in files], sr,
                                                window_seconds, context_seconds, max_batch, max_columns, save_individual_results)
        work = [file_info(i) + (sigs[i], gts[i] if known else None, hosts[i]) for i in range(F)]
    for part in (pipeline._ragged_groups(mixed, max_batch, max_columns) if F and window_seconds is None else []):
        B = len(part)
        rows = [mixed[i] for i in part]
        bits_g = [d_bits[i] for i in part]
        nb = [len(rec_bits[i]) for i in part]
        rat = [ratios[i] for i in part]
        if known:                                    # rows B .. 2B: full_noise (packed only), rows 2B .. 3B: clean + ground-truth bits
            rows += [noise[i] for i in part] + [clean[i] for i in part]
            bits_g += [d_bits[F + i] for i in part]
            nb += [0] * B + [len(gt_bits[i]) for i in part]
            rat = rat * 3
        (wave, masked, _), ns = pipeline.stage_group(rows, torch.cat(bits_g), nb, rat)
        n_long = max(ns[:B])
        rag = pipeline._group_geometry(ns[:B], device, sr, pipeline.FPS, nv=nb[:B])
        sigs = pipeline._denoise_group_staged(net, wave[:B, :n_long], masked[:B, :n_long], rag, signals=True)
        n_out = [hop * (t - 1) for t in rag.T]
        table = [(q * B + k, n_out[k], 0) for k in range(B) for q in range(4)]
        gt = None
        if known:
            wave[2 * B:].sub_(masked[2 * B:])        # silent intervals of the clean signal truly silent (M2/predict.py:321)
            gt = _round_trip(wave[B:], ns[B:])
            n_gt = [hop * (n // hop) for n in ns[B:]]
        host = None
        if save_individual_results:                  # the signals of the whole group: one unpack launch, one download
            if known:                                # ground-truth rows follow the group's 4 B rows, cropped like _write_individual
                if gt.shape[1] != sigs.shape[1]:
                    wide = torch.zeros((6 * B, max(gt.shape[1], sigs.shape[1])), dtype=torch.float32, device=device)
                    wide[:4 * B, :sigs.shape[1]] = sigs
                    wide[4 * B:, :gt.shape[1]] = gt
                    both = wide
                else:
                    both = torch.cat([sigs, gt], dim=0)
                table = [row for k in range(B) for row in
                         ([(q * B + k, n_out[k], 0) for q in range(4)] +
                          [((4 + q) * B + k, min(n_gt[q * B + k], n_out[k]), 0) for q in range(2)])]
            else:
                both = sigs
            tab = np.asarray(table, dtype=np.int64)
            tab[:, 2] = ragged.offsets(tab[:, 1])
            host = ragged.split(tools.ragged_unpack(both, tab).cpu().numpy(), tab[:, 1])
        per = 6 if known else 4
        for k, i in enumerate(part):
            data, info = file_info(i)
            sig_i = [sigs[q * B + k, :n_out[k]] for q in range(4)]
            gt_i = [gt[q * B + k, :n_gt[q * B + k]] for q in range(2)] if known else None
            host_i = host[per * k:per * (k + 1)] if host is not None else None
            work[i] = (data, info, sig_i, gt_i, host_i)
    stat = [w[1] for w in work]
    _batch_measures([w[:4] for w in work if w[3] is not None], pesq_fn, stoi_fn)
    for data, info, _, _, host_i in work:
        if host_i is not None:
            _write_individual_host(data, info, host_i[:4], host_i[4:] if known else None, outputs, snr)
    if save_stat:
        _write_eval_results(data_info, stat, outputs, threshold, snr)
    return stat
