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
the host-side bookkeeping around it.

Every stage has several forms (per file, ragged groups of files, windows); the forms differ in their compute calls and share
the bookkeeping, which is stated once per stage: the noise draw (_draw_noise, _store_crop), the decision step (_detect_item),
the recovered files (_write_recovered), the per-file records (_file_info, _data_info, _write_individual) and the two halves
of denoise_first_model (_first_model_whole, _first_model_windows)."""
import json
import os
from collections import OrderedDict, namedtuple
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


# One file of detect_files on its way from the data-set JSON to its eval_results item: its index, its JSON entry, the whole bit
# stream, the first labelled frame, the labelled frames as '0' / '1' strings, and the 14 kHz signal on the device.
Pending = namedtuple('Pending', 'data_id f bits_full i1 label snd')


def _pending_files(ds, data_root, batch_files):
    """Step 1 of detect_files, a generator of Pending: batch_files takes every recording from one audio_io.load_batch_device
    call before the first file is handed out; the per-file form decodes a file when the consumer asks for it."""
    paths = [_resolve(f['audio_path'], ds.get('dataset_path'), data_root) for f in ds['files']]
    loaded = audio_io.load_batch_device(paths, sr=DATA_REQUIRED_SR)[0] if batch_files and paths else None
    for data_id, f in enumerate(ds['files']):
        bits_full = f[BITSTREAM_JSON_LABEL]
        i1, i2 = _trim_unknown(bits_full)
        label = [str(int(b)) for b in bits_full[i1:i2]]
        snd = loaded[data_id] if batch_files else audio_io.load_device(paths[data_id], sr=DATA_REQUIRED_SR)[0]
        yield Pending(data_id, f, bits_full, i1, label, snd)


def _load_host(path):
    """A recording or noise file as a 14 kHz host array."""
    return audio_io.load(path, sr=DATA_REQUIRED_SR)[0]


def _draw_noise(rng, noise_files, load, p):
    """THE noise draw of a file (M1/dataset.py:141-142): which noise file, then -- its length is needed -- where the crop of
    ceil(duration) seconds starts.  Two draws from the seeded generator per file, in file order, whatever the form: that is why
    a seeded run stores the same crops under every form.  load(k) decodes noise file k at 14 kHz.
    -> (k, start, crop, start_pos): the crop is noise k from `start` on, and it is mixed in from its sample `start_pos` on, the
    sample of the first labelled frame."""
    k = int(rng.integers(len(noise_files)))
    noise = load(k)
    need = int(np.ceil(p.f['duration'])) * DATA_REQUIRED_SR
    start = int(rng.integers(0, max(len(noise) - need, 0) + 1))
    return k, start, noise[start:start + need], int(p.i1 / p.f['framerate'] * DATA_REQUIRED_SR)


def _store_crop(noise_dir, p, crop, snr, noise_entries):
    """The crop of a file as <noise_dir>/<name>_noise.wav and its record for create_data_from_prediction (M1/predict.py:82-104)."""
    base = os.path.basename(p.f['path'])
    stem = base.split('.mp4')[0].split('.wav')[0]
    ensure_dir(noise_dir)
    audio_io.write_wav(os.path.join(noise_dir, stem + '_noise.wav'), crop.astype(np.float32), DATA_REQUIRED_SR)
    noise_entries[base] = OrderedDict([('audio', stem + '.wav'), ('noise', stem + '_noise.wav'), ('snr', snr)])


def _mix_file(p, rng, noise_files, snr, noise_dir, noise_entries):
    """Step 2 of detect_files, per file: the recording silenced on its labelled silent intervals (M1/dataset.py:247-249) and
    mixed with its crop on the host (add_noise_to_audio); the noise file is decoded for this file alone."""
    gt = torch.tensor([int(b) for b in p.label], dtype=torch.uint8, device=p.snd.device).reshape(1, -1)
    gmask = tools.bits_to_mask_batch(gt, float(DATA_REQUIRED_SR) / p.f['framerate'], p.snd.numel())
    audio = (p.snd * (1 - gmask[0])).cpu().numpy()
    _, _, crop, start_pos = _draw_noise(rng, noise_files, lambda k: _load_host(noise_files[k]), p)
    mixed, _, _ = add_noise_to_audio(audio, crop, snr, start_pos=start_pos)
    _store_crop(noise_dir, p, crop, snr, noise_entries)
    return p._replace(snd=torch.from_numpy(np.ascontiguousarray(mixed, dtype=np.float32)).to(p.snd.device))


def _mix_pending(pending, rng, noise_files, snr, noise_dir, noise_entries, max_bytes):
    """Step 2 of detect_files(batch_mix=True): the draws per file in file order, every distinct noise file decoded once; then
    the recordings silenced on their labelled silent intervals and mixed with their crops on the device, one
    tools.add_signals_ragged call per group of files of at most max_bytes of samples."""
    noises = {}                                 # the decoded noise files by index
    which, first, count = [], [], []            # per file: its noise file, the first noise sample mixed in, the valid samples

    def load(k):
        if k not in noises:
            noises[k] = _load_host(noise_files[k])
        return noises[k]

    for p in pending:
        k, start, crop, start_pos = _draw_noise(rng, noise_files, load, p)
        which.append(k)
        first.append(start + start_pos)
        count.append(max(len(crop) - start_pos, 0))
        _store_crop(noise_dir, p, crop, snr, noise_entries)
    used = sorted(noises)
    slot = {k: j for j, k in enumerate(used)}
    out = []
    for group in ragged.byte_groups([4 * p.snd.numel() for p in pending], max_bytes):
        part = [pending[i] for i in group]
        bits = [np.asarray([int(b) for b in p.label], dtype=np.uint8) if p.label else None for p in part]
        ratios = [float(DATA_REQUIRED_SR) / p.f['framerate'] if b is not None else None for p, b in zip(part, bits)]
        mixed, _, _ = tools.add_signals_ragged([p.snd for p in part], [noises[k] for k in used], snr,
                                               noise_index=[slot[which[i]] for i in group], starts=[first[i] for i in group],
                                               counts=[count[i] for i in group], bits=bits, ratios=ratios, norm=0.5)
        out += [p._replace(snd=m) for p, m in zip(part, mixed)]
    return out


def _detect_item(p, conf, pred=None):
    """THE decision step: one `data` entry of eval_results.json (M1/predict.py:150-175) from the host array of a file's
    confidences.  The dense per-file route also hands in the kernel's bits.  The grouped and the windowed route download one
    array, sos_threshold_bits' confidence s, and leave `pred` out: the kernel's bit is s >= threshold in f32, and the same f32
    comparison on the host gives the same bit."""
    if pred is None:
        pred = (conf >= np.float32(SIGMOID_THRESHOLD)).astype(np.uint8)
    pred_label = [str(int(b)) for b in pred]
    f = p.f
    return OrderedDict([
        ('id', p.data_id), ('path', f['path']), ('full_bit_stream', p.bits_full), ('num_frames', f['num_frames']),
        ('framerate', f['framerate']), ('audio_sample_rate', f['audio_sample_rate']),
        ('audio_samples', f['audio_samples']), ('duration', f['duration']), ('frame_start_idx', p.i1),
        ('label', p.label), ('pred_label', pred_label), ('match', p.label == pred_label),
        ('confidence', [str(c) for c in conf])])


def _detect_file(net, p):
    """Step 3 of detect_files, per file: one dense detector pass over the whole recording."""
    S = transform.stft_batch(p.snd.reshape(1, -1))
    logits = net(s=S, v_num_frames=len(p.label))
    pred, conf = tools.threshold_bits(logits, SIGMOID_THRESHOLD)
    pred = pred[0].cpu().numpy()
    return _detect_item(p, conf[0].cpu().numpy(), pred)


@torch.no_grad()
def _detect_groups(net, pending, max_batch, max_columns):
    """Step 3 of detect_files(batch_files=True): the files through the detector in ragged groups, one download of confidences
    per group; the stat entries in file order."""
    from . import engine as E
    from . import pipeline
    clips = [p.snd.contiguous() for p in pending]
    items = [None] * len(pending)
    for part in pipeline._ragged_groups(clips, max_batch, max_columns):
        wave, ns = pipeline.stage_group([clips[i] for i in part])
        nv = [len(pending[i].label) for i in part]
        rag = E.Ragged([1 + n // transform.HOP_LENGTH for n in ns], wave.device, n_vframes=nv, n_samples=ns)
        S = transform.stft_batch(wave, clip_samples=rag.tab(ns))
        logits = net(s=S, v_num_frames=max(nv), rag=rag)
        _, conf = tools.threshold_bits(logits, SIGMOID_THRESHOLD)
        conf = conf.cpu().numpy()
        for k, i in enumerate(part):
            items[i] = _detect_item(pending[i], conf[k, :nv[k]])
    return items


@torch.no_grad()
def _detect_windows(net, pending, window_seconds, context_seconds, max_batch, max_columns):
    """Step 3 of detect_files(window_seconds=...): the files through pipeline.detect_long -- the recordings in overlapping
    windows, ONE stitched logit stream per file at the file's own framerate and label length -- and one thresholding launch and
    one download of confidences for all of them."""
    from . import pipeline
    nv = [len(p.label) for p in pending]
    pairs = pipeline.detect_long(net, [p.snd.contiguous() for p in pending], sr=DATA_REQUIRED_SR, fps=[p.f['framerate'] for p in pending],
                                 window_seconds=window_seconds, context_seconds=context_seconds, max_batch=max_batch,
                                 max_columns=max_columns, n_frames=nv)
    _, conf = tools.threshold_bits(torch.cat([lg for lg, _ in pairs]), SIGMOID_THRESHOLD)
    return [_detect_item(p, c) for p, c in zip(pending, ragged.split(conf.cpu().numpy(), nv))]


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
    clean_audio = noise_files is not None
    if batch_mix and not (batch_files and clean_audio):
        raise ValueError("batch_mix=True applies to noise_files given with batch_files=True")
    if clean_audio and snr is None:
        raise ValueError("the clean-recordings branch needs an snr")
    suffix = convert_snr_to_suffix2(snr) if clean_audio else ''
    noise_dir = os.path.join(os.path.abspath(outputs), 'noise' + suffix)
    noise_entries = OrderedDict()
    # 1. load.  The steps are lazy where the form is per file: a file is then loaded, mixed and detected before the next one
    files = _pending_files(ds, data_root, batch_files)
    # 2. draw and mix
    mix = (np.random.default_rng(seed), noise_files, snr, noise_dir, noise_entries)
    if batch_mix:
        files = _mix_pending(list(files), *mix, max_mix_bytes)
    elif clean_audio:
        files = (_mix_file(p, *mix) for p in files)
    # 3. detect
    if not batch_files:
        stat = [_detect_file(net, p) for p in files]
    elif window_seconds is None:
        stat = _detect_groups(net, list(files), max_batch, max_columns)
    else:
        stat = _detect_windows(net, list(files), window_seconds, context_seconds, max_batch, max_columns)
    # 4. write
    stat_dict = OrderedDict([
        ('data_total_frames', CLIP_FRAMES), ('data_center_frames', SILENT_CONSECUTIVE_FRAMES),
        ('sigmoid_threshold', SIGMOID_THRESHOLD), ('snr', snr if clean_audio else None),
        ('prediction_statistics', OrderedDict([('all', show_metrics([b for it in stat for b in it['label']],
                                                                    [b for it in stat for b in it['pred_label']]))]))])
    stat_dict['data'] = sorted(stat, key=lambda x: np.mean([float(c) for c in x['confidence']]), reverse=True)
    if clean_audio:
        with open(os.path.join(noise_dir, suffix[1:] + '.json'), 'w') as fp:
            json.dump(OrderedDict([('snrs', [snr]), ('files', noise_entries)]), fp, **JSON_DUMP_PARAMS)
    if save_stat:
        ensure_dir(os.path.abspath(outputs))
        with open(os.path.join(os.path.abspath(outputs), 'eval_results' + suffix + '.json'), 'w') as fp:
            json.dump(stat_dict, fp, **JSON_DUMP_PARAMS)
    return stat_dict


# One file of create_data_from_prediction(save_results=True): its pred_data.json item, where its recording lies on this
# machine, the directory of the recovered files and their common name.
Recovered = namedtuple('Recovered', 'item path save_dir filename')


def _write_recovered(job, mixed, clean=None, full_noise=None):
    """<name>_mixed.wav (and, with the clean-recordings branch, _clean.wav and _full_noise.wav) of a file from host arrays, and
    the item's keys that name them (M1/create_data_from_pred.py:158-190)."""
    for key, tag, y in (('mixed_audio', '_mixed', mixed), ('clean_audio', '_clean', clean), ('full_noise', '_full_noise', full_noise)):
        if y is not None:
            name = job.filename + tag + '.wav'
            audio_io.write_wav(os.path.join(job.save_dir, name), y, DATA_REQUIRED_SR)
            job.item[key] = os.path.join(os.path.basename(job.save_dir), name)
    if clean is not None:
        job.item['audio_path'] = os.path.join(job.save_dir, job.filename + '_clean.wav')


def _write_recovered_files(jobs, noise_dir, noise_files):
    """create_data_from_prediction per file: the recording (and its stored noise crop) decoded and mixed one file at a time.
    noise_files: the `files` of the noise JSON, None outside the clean-recordings branch."""
    for job in jobs:
        snd = _load_host(job.path)
        if noise_files is None:
            _write_recovered(job, snd)
            continue
        entry = noise_files[os.path.basename(job.item['path'])]
        noise = _load_host(os.path.join(noise_dir, entry['noise']))
        mixed, clean, full_noise = add_noise_to_audio(snd, noise, entry['snr'], start_pos=0, norm=0.5)
        _write_recovered(job, mixed.astype(np.float32), clean.astype(np.float32), full_noise[0].astype(np.float32))


def _write_recovered_batch(jobs, noise_dir, noise_files, max_bytes):
    """create_data_from_prediction(batch_files=True): per group of files one audio_io.load_batch_device for the recordings (and
    one for the stored noise crops, one tools.add_signals_ragged call) and one download."""
    for group in audio_io.file_groups([j.path for j in jobs], max_bytes):
        part = [jobs[i] for i in group]
        B = len(part)
        snds, _ = audio_io.load_batch_device([j.path for j in part], sr=DATA_REQUIRED_SR)
        if noise_files is None:
            host = ragged.download(snds, np.float32)
        else:
            entries = [noise_files[os.path.basename(j.item['path'])] for j in part]
            noises, _ = audio_io.load_batch_device([os.path.join(noise_dir, e['noise']) for e in entries], sr=DATA_REQUIRED_SR)
            mixed, clean, full_noise = tools.add_signals_ragged(snds, noises, [e['snr'] for e in entries], starts=0, norm=0.5)
            host = ragged.download(mixed + clean + full_noise, np.float32)
        for k, job in enumerate(part):
            _write_recovered(job, *host[k::B])                  # file-major: mixed of all files, then clean, then full_noise


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
            jobs.append(Recovered(item, _resolve(wav_path, src_root, data_root), save_dir, os.path.basename(wav_path).split('.wav')[0]))
    if jobs:
        noise_dir, noise_files = os.path.join(get_parent_dir(output_json), 'noise' + nsuffix), None
        if clean_audio:                                            # what detect_files stored: read once per call
            with open(os.path.join(noise_dir, nsuffix[1:] + '.json'), 'r') as fpn:
                noise_files = json.load(fpn)['files']
        if batch_files:
            _write_recovered_batch(jobs, noise_dir, noise_files, max_bytes)
        else:
            _write_recovered_files(jobs, noise_dir, noise_files)
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


def _gt_bits(bitstream):
    """The ground-truth bit stream as 0 / 1 values: everything but '0' is non-silent (M2/predict.py:318-320)."""
    return [0 if b == '0' else 1 for b in bitstream]


# The keys of a file that travel from pred_data.json into its stat.json / eval_results entry, in the order the reference
# writes them; those in _KNOWN_ONLY (of the info record, or of an item of get_data_from_first_model) exist with a known clean signal (unknown_clean_signal=False) alone.
_INFO_KEYS = ('id', 'path', 'clean_audio_path', 'mixed_audio_path', 'full_noise_path', 'bitstream', 'sr', 'snr')
_KNOWN_ONLY = ('clean_audio_path', 'full_noise_path', 'clean', 'full_noise')


def _file_info(data):
    """The ordered `info` record of a file (M2/predict.py:430-450) from whatever of _INFO_KEYS its `data` carries."""
    info = OrderedDict((k, data[k]) for k in _INFO_KEYS if k in data)
    info['id'], info['path'] = str(info['id']), str(info['path'])
    return info


def _data_info(obj):
    """What eval_results.json of stage 2 repeats of pred_data.json."""
    return OrderedDict([(k, obj[k]) for k in ('dataset_path', 'num_videos', 'data_total_frames', 'data_center_frames',
                                              'sigmoid_threshold')])


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
    base = get_parent_dir(first_model_json_path)
    stft = lambda y: transform.stft_batch(y.reshape(1, -1), n_fft, hop_length, win_length)      # noqa: E731
    data_list = []
    for data in obj['files']:
        mixed_audio_path = os.path.join(base, data['mixed_audio'])
        mixed_sig, _ = audio_io.load_device(mixed_audio_path, sr=sr)
        bitstream = data[BIT_STREAM_LABEL]
        bits = torch.tensor(_parse_bits(bitstream), dtype=torch.uint8, device=mixed_sig.device).reshape(1, -1)
        mask, noise_sig = tools.bits_to_mask_batch(bits, float(sr) / data['framerate'], mixed_sig.numel(),
                                                   mixed_sig.reshape(1, -1))
        clean_audio_path = full_noise_path = clean = full_noise = None
        if not unknown_clean_signal:
            clean_audio_path, full_noise_path = os.path.join(base, data['clean_audio']), os.path.join(base, data['full_noise'])
            clean_sig, _ = audio_io.load_device(clean_audio_path, sr=sr)
            full_noise_sig, _ = audio_io.load_device(full_noise_path, sr=sr)
            gt = torch.tensor(_gt_bits(data[GT_BIT_STREAM_LABEL]), dtype=torch.uint8, device=clean_sig.device).reshape(1, -1)
            gt_mask = tools.bits_to_mask_batch(gt, float(sr) / data['framerate'], clean_sig.numel())
            clean = stft(clean_sig * (1 - gt_mask[0]))           # silent intervals truly silent (M2/predict.py:321)
            full_noise = stft(full_noise_sig)
        item = OrderedDict([
            ('id', os.path.splitext(os.path.basename(data['path']))[0]), ('path', data['path']),
            ('clean_audio_path', clean_audio_path), ('mixed_audio_path', mixed_audio_path), ('full_noise_path', full_noise_path),
            ('bitstream', bitstream), ('mixed', stft(mixed_sig)), ('clean', clean), ('noise', stft(noise_sig)),
            ('full_noise', full_noise), ('mask', mask[0]), ('snr', snr), ('sr', sr)])
        if unknown_clean_signal:
            for k in _KNOWN_ONLY:
                del item[k]
        data_list.append(item)
    return data_list, _data_info(obj)


# One file of stage 2 after the denoiser: its `data` (id, sr, ...) and `info` records, the four signals (noisy input, noise
# intervals, predicted full noise, denoised output) and, with a known clean signal, the two ground-truth ones (full noise,
# clean input) on the device, or None; host: the same four (six) signals as host arrays where a form has downloaded them.
Denoised = namedtuple('Denoised', 'data info sigs gt_sigs host')


def _write_individual(w, outputs, snr):
    """The WAVE files and stat.json of one file of stage 2 (M2/predict.py:515-560); fills the path keys of its `info`.  A form
    that has not downloaded the signals of its files in one copy leaves `host` None: they come down here."""
    if w.host is not None:
        host, gh = w.host[:4], (w.host[4:] if len(w.host) > 4 else None)
    else:
        host, gh = w.sigs.cpu().numpy(), (None if w.gt_sigs is None else w.gt_sigs.cpu().numpy())
    save_dir = os.path.join(os.path.abspath(outputs), convert_snr_to_suffix2(snr)[1:], str(w.data['id']))
    ensure_dir(save_dir)
    named = list(zip(('noisy_input', 'noise_intervals', 'predicted_full_noise', 'denoised_output'), host))
    if gh is not None:
        named += [(name, g[:len(host[0])]) for name, g in zip(('ground_truth_full_noise', 'ground_truth_clean_input'), gh)]
    for name, y in named:
        p = os.path.join(save_dir, name + '.wav')
        audio_io.write_wav(p, y, w.data['sr'])
        w.info[name] = p
    with open(os.path.join(save_dir, 'stat.json'), 'w') as fp:
        json.dump(w.info, fp, **JSON_DUMP_PARAMS)


def _batch_measures(work, pesq_fn, stoi_fn):
    """The objective measures of all files with a known clean signal (denoise_files(batch_metrics=True)): outputs and clean
    signals to 16 kHz in one resample_batch_device call per distinct rate (2 F clips), one evaluate_metrics_batch."""
    work = [w for w in work if w.gt_sigs is not None]
    if not work:
        return
    out16, clean16 = [None] * len(work), [None] * len(work)
    by_rate = OrderedDict()
    for i, w in enumerate(work):
        by_rate.setdefault(w.data['sr'], []).append(i)
    for sr, idx in by_rate.items():
        clips = [work[i].sigs[3].contiguous() for i in idx] + [work[i].gt_sigs[1].contiguous() for i in idx]
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
    for w, m in zip(work, metrics.evaluate_metrics_batch(out16, clean16, sr=16000, pesq=pesq, stoi=stoi)):
        w.info.update(m)


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
        info = _file_info(data)
        gt_sigs = None
        if 'clean' in data:
            gt_sigs = transform.istft_batch(torch.cat([data['full_noise'], data['clean']], dim=0))
            if not batch_metrics:
                out16 = audio_io.resample_device(sigs[3].contiguous(), data['sr'], 16000)
                clean16 = audio_io.resample_device(gt_sigs[1].contiguous(), data['sr'], 16000)
                pesq = pesq_fn(clean16.cpu().numpy(), out16.cpu().numpy(), 16000) if pesq_fn is not None else None
                stoi = stoi_fn(clean16.cpu().numpy(), out16.cpu().numpy(), 16000) if stoi_fn is not None else None
                info.update(metrics.evaluate_metrics(out16, clean16, sr=16000, pesq=pesq, stoi=stoi))
        stat.append(info)
        w = Denoised(data, info, sigs, gt_sigs, None)
        if batch_metrics:
            work.append(w)
        elif save_individual_results:
            _write_individual(w, outputs, snr)
    _batch_measures(work, pesq_fn, stoi_fn)
    for w in work if save_individual_results else []:
        _write_individual(w, outputs, snr)
    if save_stat:
        _write_eval_results(data_info, stat, outputs, threshold, snr)
    return stat


def _round_trip(wave, ns):
    """STFT -> ISTFT of the rows of a padded buffer, every row at its own `ns` samples (hop * (n // hop) come back)."""
    from . import engine as E
    rag = E.Ragged([1 + n // transform.HOP_LENGTH for n in ns], wave.device, n_samples=ns)
    return transform.istft_batch(transform.stft_batch(wave, clip_samples=rag.tab(ns)), clip_frames=rag.level(0))


def _rows_under(a, b):
    """The rows of `b` under the rows of `a` in one f32 buffer, the narrower of the two zero-filled to the other's width."""
    if a.shape[1] == b.shape[1]:
        return torch.cat([a, b], dim=0)
    wide = torch.zeros((a.shape[0] + b.shape[0], max(a.shape[1], b.shape[1])), dtype=torch.float32, device=a.device)
    wide[:a.shape[0], :a.shape[1]] = a
    wide[a.shape[0]:, :b.shape[1]] = b
    return wide


def _first_model_whole(net, mixed, noise, clean, all_bits, nb, ngt, ratios, sr, max_batch, max_columns, download):
    """The whole-file half of denoise_first_model, with the arguments and the result of _first_model_windows (below).
    The files sorted by length and cut into groups (pipeline._ragged_groups); a group is staged by ONE sos_ragged_stage_f32
    launch and runs as pipeline.denoise_ragged(bits=..., return_all=True) runs it.  With known clean signals the group has
    2 B more rows: B .. 2 B full_noise (packed only), 2 B .. 3 B the clean recordings with their ground-truth decisions, whose
    mask comes out of the same launch; their STFT -> ISTFT round trips are the ground-truth signals.  With `download` the four
    (six) signals of every file of a group come down in one copy (sos_ragged_unpack_f32), the ground-truth ones cropped to the
    output length."""
    from . import pipeline
    F, device, hop, known = len(mixed), mixed[0].device, transform.HOP_LENGTH, bool(noise)
    d_bits = ragged.split(all_bits, list(nb) + list(ngt))
    sigs, gts, hosts = [None] * F, [None] * F, [None] * F
    for part in pipeline._ragged_groups(mixed, max_batch, max_columns):
        B = len(part)
        rows = [mixed[i] for i in part]
        bits_g = [d_bits[i] for i in part]
        nbits = [nb[i] for i in part]
        rat = [ratios[i] for i in part]
        if known:
            rows += [noise[i] for i in part] + [clean[i] for i in part]
            bits_g += [d_bits[F + i] for i in part]
            nbits += [0] * B + [ngt[i] for i in part]
            rat = rat * 3
        (wave, masked, _), ns = pipeline.stage_group(rows, torch.cat(bits_g), nbits, rat)
        n_long = max(ns[:B])
        rag = pipeline._group_geometry(ns[:B], device, sr, pipeline.FPS, nv=nbits[:B])
        out = pipeline._denoise_group_staged(net, wave[:B, :n_long], masked[:B, :n_long], rag, signals=True)
        n_out = [hop * (t - 1) for t in rag.T]
        take = [[(q * B + k, n_out[k], 0) for q in range(4)] for k in range(B)]        # per file: (row, samples, -) to unpack
        if known:
            wave[2 * B:].sub_(masked[2 * B:])        # silent intervals of the clean signal truly silent (M2/predict.py:321)
            gt = _round_trip(wave[B:], ns[B:])
            n_gt = [hop * (n // hop) for n in ns[B:]]
            for k in range(B):                       # the ground-truth rows follow the group's 4 B rows
                take[k] += [((4 + q) * B + k, min(n_gt[q * B + k], n_out[k]), 0) for q in range(2)]
        if download:                                 # the signals of the whole group: one unpack launch, one download
            tab = np.asarray([row for rows_k in take for row in rows_k], dtype=np.int64)
            tab[:, 2] = ragged.offsets(tab[:, 1])
            host = ragged.split(tools.ragged_unpack(_rows_under(out, gt) if known else out, tab).cpu().numpy(), tab[:, 1])
        per = len(take[0])
        for k, i in enumerate(part):
            sigs[i] = [out[q * B + k, :n_out[k]] for q in range(4)]
            if known:
                gts[i] = [gt[q * B + k, :n_gt[q * B + k]] for q in range(2)]
            if download:
                hosts[i] = host[per * k:per * (k + 1)]
    return sigs, gts, hosts


def _first_model_windows(net, mixed, noise, clean, all_bits, nb, ngt, ratios, sr, max_batch, max_columns, download,
                         framerates, window_seconds, context_seconds):
    """The windowed half of denoise_first_model: `mixed` (one 1-D GPU recording per file; `noise` / `clean`: the ground-truth
    recordings or empty lists), all_bits = the files' `recovered_prediction` decisions (nb each) followed by the ground-truth
    ones (ngt each) in one GPU buffer.  -> per file ([4 signals], [2 ground-truth signals] or None, host arrays of the
    4 (6) signals as _write_individual takes them, or None without `download`).
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

    def four(b, i):
        return [b[base[i] + q * pitch[i]:base[i] + q * pitch[i] + lens[i]] for q in range(4)]

    sigs = [four(buf, i) for i in range(F)]
    hosts = [four(host, i) if download else None for i in range(F)]
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
    if download:                                                 # cropped like the whole-file half: one more copy
        gh = ragged.download([g[:lens[i]] for i in range(F) for g in gts[i]])
        hosts = [hosts[i] + gh[2 * i:2 * i + 2] for i in range(F)]
    return sigs, gts, hosts


def _check_frames(paths, ys, sr, what):
    """ValueError naming the first file with fewer STFT frames than the denoiser takes."""
    from . import pipeline
    hop = transform.HOP_LENGTH
    for path, y in zip(paths, ys):
        if 1 + y.numel() // hop < pipeline.MIN_FRAMES:
            raise ValueError("%s: %d samples at %d Hz are fewer than the %d STFT frames (%d samples) %s needs"
                             % (path, y.numel(), sr, pipeline.MIN_FRAMES, pipeline.MIN_FRAMES * hop, what))


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
    # 1. parse
    with open(first_model_json_path, 'r') as fp:
        obj = json.load(fp)
    base = get_parent_dir(first_model_json_path)
    files = obj['files']
    known = not unknown_clean_signal
    F = len(files)
    data_info = _data_info(obj)
    data_info['snr'] = snr
    net.eval()
    mixed_paths = [os.path.join(base, d['mixed_audio']) for d in files]
    clean_paths = [os.path.join(base, d['clean_audio']) for d in files] if known else []
    noise_paths = [os.path.join(base, d['full_noise']) for d in files] if known else []
    rec_bits = [np.asarray(_parse_bits(d[BIT_STREAM_LABEL]), dtype=np.uint8) for d in files]
    gt_bits = [np.asarray(_gt_bits(d[GT_BIT_STREAM_LABEL]), dtype=np.uint8) for d in files] if known else []
    datas = [dict(id=os.path.splitext(os.path.basename(d['path']))[0], path=d['path'], mixed_audio_path=mixed_paths[i],
                  bitstream=d[BIT_STREAM_LABEL], sr=sr, snr=obj['snr']) for i, d in enumerate(files)]
    for data, c, n in zip(datas, clean_paths, noise_paths):
        data.update(clean_audio_path=c, full_noise_path=n)
    work = []
    if F:
        # 2. load
        ys, _ = audio_io.load_batch_device(mixed_paths + clean_paths + noise_paths, sr=sr)
        mixed, clean, noise = ys[:F], ys[F:2 * F], ys[2 * F:]
        # 3. check
        _check_frames(mixed_paths, mixed, sr, "the denoiser")
        if window_seconds is not None:                     # the ground-truth recordings are windowed under a plan of their own
            _check_frames(clean_paths + noise_paths, clean + noise, sr, "a window")
        # 4. one of the two halves
        all_bits = torch.from_numpy(np.concatenate(rec_bits + gt_bits)).to(mixed[0].device)       # every bit string: one copy
        args = (net, mixed, noise, clean, all_bits, [len(b) for b in rec_bits], [len(b) for b in gt_bits],
                [float(sr) / d['framerate'] for d in files], sr, max_batch, max_columns, save_individual_results)
        if window_seconds is None:
            halves = _first_model_whole(*args)
        else:
            halves = _first_model_windows(*args, [d['framerate'] for d in files], window_seconds, context_seconds)
        work = [Denoised(data, _file_info(data), *half) for data, *half in zip(datas, *halves)]
    # 5. measure
    _batch_measures(work, pesq_fn, stoi_fn)
    # 6. write
    for w in work if save_individual_results else []:
        _write_individual(w, outputs, snr)
    stat = [w.info for w in work]
    if save_stat:
        _write_eval_results(data_info, stat, outputs, threshold, snr)
    return stat
