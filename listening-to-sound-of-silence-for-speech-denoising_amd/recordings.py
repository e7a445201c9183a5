"""Recordings in, denoised recordings out: WAVE files of any channel count, rate and sample format through the chain of
windows.denoise_long and back into files with the SAME number of frames, channels, rate and sample format.  By default every
channel is denoised on its own; link_channels='any' / 'mean' silences the channels of a file by ONE stream of decisions shared
between them (windows.denoise_long(stitch_bits=True, link=): one sos_window_frames_link_f32 launch for all files of a group), so
that the noise floors of a stereo pair drop in and out together.  The decode, the two resamplings, the windows
and the encode each run in launches shared by all files and channels of a group (csrc/pcm_io.hip, csrc/wave_io.hip,
csrc/ragged_window.hip).  The networks run at 14 kHz: by default a file of a higher rate comes back band-limited to 7 kHz;
high_band='keep' / 'follow' merge the band above 7 kHz of the source back in (csrc/band_merge.hip).  loudness= brings every
written file to a target integrated loudness (ITU-R BS.1770 / EBU R128, csrc/loudness.hip) by one gain per file before the encode;
peak='true' states its ceiling in dBTP and loudness_range=True reports the loudness range and the R128 maxima;
limiter='lookahead' holds the peaks at the ceiling by a gain that dips around them only (csrc/limiter.hip), so that a file whose
peaks would bind the one gain still reaches its target."""
import os

import numpy as np
import torch

from . import audio_io
from . import labels
from . import metrics
from . import ragged
from . import tools
from . import transform
from . import wave_file
from . import windows
from .pipeline import FPS, MIN_FRAMES, SR

# the format a source is written back in: (WAVE format tag, stored bits) -> audio_io.ENCODINGS / G711 name.  A float64 source is
# written as f32 (the networks compute in f32 at best); a G.711 source (telephone audio) comes back as G.711 of its own law.
_SOURCE_FORMAT = {source: f.back for source, f in wave_file.SOURCES.items()}
SAMPLE_FORMATS = {**audio_io.ENCODINGS, **audio_io.G711}         # name -> (code, bytes per element, WAVE format tag, bits)


def _model_samples(frames, rate):
    """Samples of a channel of `frames` frames at `rate` once it is at the networks' rate (resample_batch_device's length)."""
    return int(frames) if rate == SR else int(np.ceil(int(frames) * (float(SR) / rate)))


HIGH_BAND_MODES = ("drop", "keep", "follow")


def _check_files(paths, out_dir, sample_format, suffix, link_channels=None, high_band="drop", smooth_frames=2):
    """Everything that can be refused from the arguments and the chunk headers alone: -> (infos, formats, out_paths)."""
    if high_band not in HIGH_BAND_MODES:
        raise ValueError("denoise_recordings: unknown high_band %r (one of %s)" % (high_band, ", ".join(HIGH_BAND_MODES)))
    if isinstance(smooth_frames, bool) or not isinstance(smooth_frames, (int, np.integer)) or not 0 <= smooth_frames <= 16:
        raise ValueError("denoise_recordings: smooth_frames is a whole number of frames within 0 .. 16, got %r" % (smooth_frames,))
    if link_channels is not None and link_channels not in tools.LINK_MODES:
        raise ValueError("denoise_recordings: unknown link_channels %r (None, or one of %s)"
                         % (link_channels, ", ".join(sorted(tools.LINK_MODES))))
    if sample_format is not None and sample_format not in SAMPLE_FORMATS:
        raise ValueError("denoise_recordings: unsupported sample_format %r (one of %s)"
                         % (sample_format, ", ".join(sorted(SAMPLE_FORMATS))))
    infos, formats, out_paths = [], [], []
    hop = transform.HOP_LENGTH
    for path in paths:
        info = audio_io.wave_info(path)                 # WaveFormatError (a ValueError) names the file: format, channels
        n = _model_samples(info["frames"], info["rate"]) if info["rate"] > 0 else 0
        if 1 + n // hop < MIN_FRAMES:
            raise ValueError("%s: recordings need at least %d STFT frames (%d samples at %d Hz); got %d frames at %d Hz = %d samples"
                             % (path, MIN_FRAMES, MIN_FRAMES * hop, SR, info["frames"], info["rate"], n))
        if info["channels"] > 64:
            raise ValueError("%s: %d channels (at most 64)" % (path, info["channels"]))
        infos.append(info)
        formats.append(sample_format or _SOURCE_FORMAT[(info["tag"], info["bits"])])
        out_paths.append(os.path.join(out_dir, os.path.splitext(os.path.basename(path))[0] + suffix + ".wav"))
    if len(set(out_paths)) != len(out_paths):
        raise ValueError("denoise_recordings: two inputs share a file name and would be written to the same output")
    return infos, formats, out_paths


PEAK_MODES = ("sample", "true")
LIMITERS = ("lookahead",)


def _check_limiter(limiter, lookahead_ms, loudness, infos, paths):
    """What can be refused from the limiter's arguments and the files' rates: -> H per file (None without a limiter)."""
    if limiter is not None and limiter not in LIMITERS:
        raise ValueError("denoise_recordings: unknown limiter %r (None, or one of %s)" % (limiter, ", ".join(LIMITERS)))
    ok = not isinstance(lookahead_ms, (bool, str)) and np.ndim(lookahead_ms) == 0 and np.isfinite(float(lookahead_ms))
    if not ok or float(lookahead_ms) <= 0.0:
        raise ValueError("denoise_recordings: lookahead_ms is a finite number of milliseconds above 0, got %r" % (lookahead_ms,))
    if limiter is None:
        return None
    if loudness is None:
        raise ValueError("denoise_recordings: limiter=%r needs a loudness target (a number or 'source')" % (limiter,))
    hs = [int(round(float(lookahead_ms) * i["rate"] / 1000.0)) for i in infos]
    for h, i, p in zip(hs, infos, paths):
        if not 1 <= h <= audio_io.LIMITER_MAX_LOOKAHEAD:
            raise ValueError("%s: %r ms at %d Hz is a look-ahead of %d samples (1 .. %d)"
                             % (p, lookahead_ms, i["rate"], h, audio_io.LIMITER_MAX_LOOKAHEAD))
    return hs


def _check_loudness(loudness, peak_ceiling_db, channel_weights, peak="sample", loudness_range=False):
    """What can be refused from the levelling arguments alone."""
    if peak not in PEAK_MODES:
        raise ValueError("denoise_recordings: unknown peak %r (one of %s)" % (peak, ", ".join(PEAK_MODES)))
    if not isinstance(loudness_range, (bool, np.bool_)):
        raise ValueError("denoise_recordings: loudness_range is True or False, got %r" % (loudness_range,))
    if loudness is None:
        if peak == "true" or loudness_range:            # both ride the levelling's measurement, and the ceiling needs its gain
            raise ValueError("denoise_recordings: peak='true' and loudness_range=True need a loudness target (a number or 'source')")
        return
    if loudness != "source":
        ok = not isinstance(loudness, (bool, str)) and np.ndim(loudness) == 0 and np.isfinite(float(loudness))
        if not ok or not -70.0 <= float(loudness) <= 0.0:
            raise ValueError("denoise_recordings: loudness is None, 'source' or a target within -70 .. 0 LUFS, got %r" % (loudness,))
    ok = not isinstance(peak_ceiling_db, (bool, str)) and np.ndim(peak_ceiling_db) == 0 and np.isfinite(float(peak_ceiling_db))
    if not ok or float(peak_ceiling_db) > 0.0:
        raise ValueError("denoise_recordings: peak_ceiling_db is a finite level of at most 0 dBFS, got %r" % (peak_ceiling_db,))
    if channel_weights is not None:
        tables = channel_weights.values() if isinstance(channel_weights, dict) else [channel_weights]
        for w in tables:
            w = np.asarray(w, dtype=np.float64)
            if w.ndim != 1 or not 1 <= w.size <= 64 or not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError("denoise_recordings: channel_weights holds 1 .. 64 finite weights >= 0, got %r" % (w.tolist(),))
        if isinstance(channel_weights, dict):
            for k, w in channel_weights.items():
                if len(w) != k:
                    raise ValueError("denoise_recordings: channel_weights[%r] holds %d weights" % (k, len(w)))


def _file_weights(channel_weights, infos, paths):
    """The weights of every file (None: all 1.0): a sequence serves every file and must have its channel count, a dict
    {channels: weights} the files of that many channels."""
    if channel_weights is None:
        return [None] * len(infos)
    if isinstance(channel_weights, dict):
        return [channel_weights.get(i["channels"]) for i in infos]
    for i, p in zip(infos, paths):
        if i["channels"] != len(channel_weights):
            raise ValueError("%s: %d channels, but channel_weights holds %d weights (give {channels: weights} for a folder of "
                             "mixed layouts)" % (p, i["channels"], len(channel_weights)))
    return [channel_weights] * len(infos)


def _resample_back(clips, rates):
    """Every clip whose file's rate differs from SR back to that rate: one resample_batch_device launch per rate."""
    return ragged.per_group(clips, rates, lambda r, idx: audio_io.resample_batch_device([clips[k] for k in idx], SR, r),
                            lambda k, r: r == SR)


def _to_model_rate(natives, rates):
    """Every native channel at the networks' rate, as load_channels_batch_device(sr=SR) brings it there: one
    resample_batch_device launch per rate other than SR, the same bits."""
    return ragged.per_group(natives, rates, lambda r, idx: audio_io.resample_batch_device([natives[k] for k in idx], r, SR),
                            lambda k, r: r == SR)


def _merge_back(natives, lows_in, lows_out, rates, high_band, smooth_frames):
    """Every channel whose file's rate exceeds SR back at that rate WITH the band above SR / 2 (audio_io.resample_merge_batch_
    device): per rate one gains launch ('follow' only) and one merge launch.  The other channels pass as they are."""
    def merged(r, idx):
        a, b = [lows_in[k] for k in idx], [lows_out[k] for k in idx]
        gains = audio_io.band_gains_batch_device(a, b, transform.HOP_LENGTH, smooth_frames) if high_band == "follow" else None
        return audio_io.resample_merge_batch_device([natives[k] for k in idx], a, b, SR, r, gains)

    return ragged.per_group(lows_out, rates, merged, lambda k, r: r <= SR)


@torch.no_grad()
def denoise_recordings(detector, denoiser, paths, out_dir, window_seconds=30.0, context_seconds=2.0, max_batch=256,
                       max_columns=65536, max_bytes=labels.DEFAULT_MAX_BYTES, sample_format=None, suffix="", link_channels=None,
                       high_band="drop", smooth_frames=2, loudness=None, peak_ceiling_db=-1.0, channel_weights=None,
                       peak="sample", loudness_range=False, dither=None, dither_seed=0, limiter=None, lookahead_ms=5.0):
    """Denoises the WAVE files `paths` into out_dir/<name><suffix>.wav.  A written file has exactly the source's frame count,
    channels, rate and sample format (PCM 8 / 16 / 24 / 32 bit, float 32, G.711 A-law / mu-law; a float64 source is written as
    float32); sample_format= ('s16', 's24', 's32', 'u8', 'f32', 'alaw', 'ulaw') forces one format for all files.
    Per group of files of at most `max_bytes` of decoded f32 samples (ragged.byte_groups): the files are parsed on the host;
    one upload and one sos_pcm_planes_batch_f32 (G.711: sos_g711_planes_batch_f32) launch per sample format decode every channel
    into its own plane; one
    resample_batch_device launch per native rate other than 14 kHz brings all channels to the networks' rate; ONE
    windows.denoise_long call runs all channels of all files of the group as recordings (file order, channel order within a
    file; window_seconds, context_seconds, max_batch, max_columns as there); one resample launch per native rate goes back; one
    sos_pcm_encode_batch (sos_g711_encode_batch) launch per output format crops or zero-fills every channel to the source's
    frame count (the networks return hop * (n // hop) samples and the resampler ceil(n * ratio)) and quantises it -- round half
    to even, saturating, without dither unless dither= asks for it (below); G.711 compresses that s16 value and zero-fills with the code of silence; one download brings the group's bytes and counts to the host, and only then are its files written
    (audio_io.wave_container).  No call in the loop waits for the device except that download.
    link_channels: None -- every channel gets its own silent-interval decisions, per window (denoise_long's default mode) -- or
    'any' / 'mean': the channels of a file share ONE decision stream, the group's denoise_long call runs with stitch_bits=True,
    link=<the file of each channel>, link_mode=link_channels ('any': a frame is speech if any channel has speech, so noise is
    only estimated where every channel is silent; 'mean': the mean logit decides).  A mono file is a group of one.
    high_band: the networks run at 14 kHz, so what a 44.1 / 48 kHz source holds above 7 kHz never reaches them.  'drop' (the
    default) leaves it out: the written file has the source's rate and is BAND-LIMITED TO 7 kHz.  'keep' and 'follow' put it back,
    per channel of a file whose rate exceeds 14 kHz, with x the native plane, a = x at 14 kHz, b = the networks' output and U
    the resampling back: out[t] = fmaf(g[t], x[t] - U(a)[t], U(b)[t]) (csrc/band_merge.hip; one
    audio_io.resample_merge_batch_device launch per native rate instead of the resample launch back).  'keep': g = 1, the band
    above 7 kHz passes untouched, its noise included.  'follow': g follows what the networks did to the low band -- per hop
    frame min(1, sqrt(energy of b / energy of a)), averaged over 2 * smooth_frames + 1 frames (0 .. 16; 2 is about 56 ms) and
    interpolated between frame centres (audio_io.band_gains_batch_device, one more launch per rate) -- so hiss above 7 kHz drops
    in the silent intervals too; it assumes the high band's noise comes and goes with the low band's.  The last < hop samples
    at 14 kHz have no output of the networks (zero-filled today): 'follow' fades the high band out there, 'keep' leaves it in.
    Files at 14 kHz or below have no such band and are written with the same bytes under every mode.
    loudness: None (the default: nothing below runs and the written bytes are what they were), a target in LUFS (-70 .. 0) or
    'source'.  Removing the noise changes a file's level; with a target every written file is brought to that INTEGRATED
    LOUDNESS (ITU-R BS.1770-4 / EBU R128, gated: metrics.loudness_batch, csrc/loudness.hip), measured on the planes exactly as
    the encode reads them (cropped / zero-filled to the source's frame count), just before the encode: one measuring launch
    sequence and one gain launch per group (audio_io.loudness_gain_batch_device), the planes scaled by ONE float32 gain per
    file before any encoder sees them -- every output format, G.711 included, so the integer formats keep their single
    rounding.  g = min(10^((target - L) / 20), 10^(peak_ceiling_db / 20) / sample peak); peak_ceiling_db (default -1 dBFS, at
    most 0) bounds the SAMPLE peak, not the true peak; a file without a block above the gates keeps g = 1.  'source': each
    file's target is the integrated loudness of its own decoded source at its native rate (the group then keeps the native
    planes, as high_band does, and measures them in the same launch sequence as the outputs); a silent source leaves g = 1.
    channel_weights: None (every channel counts 1.0: exact for mono and stereo), one weight >= 0 per channel for all files, or
    {channels: weights} (surround: 1.41 for the rear pair and 0 for the LFE are the caller's to pass).  The rows join the
    group's one download.
    peak: 'sample' (the default) or 'true'.  'true' states the ceiling as EBU R128 does, in dBTP: the TRUE peak of the planes the
    encode will read (metrics.true_peak_batch: 4x interpolation, csrc/loudness.hip, one more launch sequence in the group's
    measurement) takes the sample peak's place in g, so the written file's true peak is at most the ceiling where a sample-peak
    ceiling can leave it up to 3 dB above (a sine at a quarter of the rate).  It needs a loudness target.
    loudness_range=True also measures the loudness range (LRA, EBU Tech 3342) and the maximum momentary / short-term loudness of
    every written file (metrics.loudness_batch(loudness_range=True): two more launches from the energies the measurement left
    on the device).  It needs a loudness target too.  Under 'source' the extra measures are taken on the outputs only (the
    sources then get a measuring sequence of their own).  Both ride the group's one download.
    dither: None (the default: plain rounding, the written bytes are what they were), 'tpdf' or 'highpass'.  The files written
    as 'u8', 's16' or 's24' get that dither before their one rounding (audio_io.encode_batch_device(dither=): drawn inside the
    encode kernel from (dither_seed, the file's position in `paths`, channel, frame), so what the denoiser pushed below one LSB
    -- the intervals between words above all, and more of it after a levelling gain below 1 -- is kept as signal under a noise
    floor free of it, not turned into distortion or gated to zero; 'highpass' moves the dither's power towards fs / 2).  The key is
    the position in `paths`, not in the group: a file's bytes do not depend on max_bytes or on the other files.  Files written
    as 's32', 'f32' or G.711 are written as before.  Still one encode launch per format and group, and one download.
    dither_seed: 0 .. 2^64 - 1; the same call twice writes the same files.
    limiter: None (the default: the launches, the bytes and the result keys are what they were) or 'lookahead'.  The one gain is
    min(to the target, ceiling / peak): where the ceiling binds, the file is written QUIETER than its target, by an amount a single
    plosive or click decides -- and denoised speech has a high crest, the floor between the words being gone.  'lookahead' (it
    needs a loudness target) applies the gain to the target in full and holds the peaks at the ceiling by a gain curve that
    dips around them only, one curve for all channels of a file (audio_io.limit_batch_device, csrc/limiter.hip: symmetric linear
    ramps over 2 * lookahead_ms on either side of a peak).  Per group: the measurement as above; the limiter (the sample or the
    true-peak envelope, as peak= says); the measurement AGAIN on the limited planes, with the true peak and the range if asked for
    (a limiter moves them); the one gain with the target set to the loudness just measured, which makes it a pure TRIM min(1,
    ceiling / peak) -- it holds the ceiling as strictly as without the limiter and takes up what a gain that varies between two
    samples leaves of a true peak; the encode.  Everything still rides the group's one download.  lookahead_ms (default 5):
    round(lookahead_ms * rate / 1000) samples, 1 .. 1024 at every file's rate.  The loudness a limiter takes away is NOT made up
    for by a second pass: `loudness` reports what was written.
    -> one dict per file: path, out_path, channels, rate, frames, format, clipped (samples that saturated or were NaN, all
    channels), windows (denoise_long windows, all channels); with loudness also loudness_before (LUFS of the denoised file
    before the gain, -inf without a gated block), loudness (before + 20 log10 g, not measured again), loudness_target, gain_db
    and peak_limited (the ceiling bound the gain); under peak='true' also true_peak_db (20 log10(g * true peak): the level
    written, in dBTP, -inf for a silent file); under loudness_range=True also lra (LU, of the planes before the gain, which a gain
    does not move) and max_momentary / max_short_term (LUFS, as written: measured before the gain, + gain_db).
    With dither= also dither: the kind, or None for a file it did not apply to.
    With limiter= the rows change: gain_db = 20 log10(the gain to the target) + the trim; loudness = the loudness MEASURED on the
    limited planes + the trim; peak_limited says the trim engaged; limiter_db (20 log10 of the least gain of the curve, at most 0)
    and limiter_samples (samples per channel the curve lowered) are new; true_peak_db, lra, max_momentary and max_short_term are
    those of the limited planes, as written.
    ValueError before any launch of the call, naming the file: fewer than MIN_FRAMES STFT frames at 14 kHz, an unsupported
    format (audio_io.WaveFormatError), no channels or more than 64, two inputs with one output name; an unknown sample_format, link_channels or
    high_band, smooth_frames outside 0 .. 16; a loudness that is not finite or outside -70 .. 0, a ceiling above 0, weights that are
    negative or not one per channel, an unknown peak, a loudness_range that is no bool, either of the two without a loudness target;
    an unknown dither, a dither_seed that is no integer in 0 .. 2^64 - 1; an unknown limiter, a limiter without a loudness target, a
    lookahead_ms that is not finite and positive, a file whose rate puts the look-ahead outside 1 .. 1024 samples;
    window_plan's argument rules; a group with more than 65535 windows."""
    paths = [os.fspath(p) for p in paths]
    if dither is not None and dither not in audio_io.DITHER:
        raise ValueError("denoise_recordings: unknown dither %r (None, or one of %s)" % (dither, ", ".join(sorted(audio_io.DITHER))))
    if isinstance(dither_seed, bool) or not isinstance(dither_seed, (int, np.integer)) or not 0 <= int(dither_seed) < 1 << 64:
        raise ValueError("denoise_recordings: dither_seed is an integer in 0 .. 2^64 - 1, got %r" % (dither_seed,))
    _check_loudness(loudness, peak_ceiling_db, channel_weights, peak, loudness_range)
    infos, formats, out_paths = _check_files(paths, out_dir, sample_format, suffix, link_channels, high_band, smooth_frames)
    _check_limiter(limiter, lookahead_ms, loudness, infos, paths)
    flags = dict(true_peak=True) if peak == "true" else {}
    if loudness_range:
        flags["loudness_range"] = True                  # with neither, loudness_batch is called as it always was
    weights = _file_weights(channel_weights, infos, paths) if loudness is not None else None
    core, context = windows._hops(round(window_seconds * SR)), windows._hops(round(context_seconds * SR))
    groups = ragged.byte_groups([4 * i["frames"] * i["channels"] for i in infos], max_bytes)
    plans = []                                          # host only: refuses bad window arguments and a group of too many windows
    for group in groups:
        plans.append(windows.window_plan([_model_samples(infos[f]["frames"], infos[f]["rate"]) for f in group
                                          for _ in range(infos[f]["channels"])], core, context))
        if len(plans[-1]) > ragged.MAX_CLIPS:
            raise ValueError("denoise_recordings: the group of %s .. %s has %d windows over all channels (at most %d): lower max_bytes "
                             "or use longer windows" % (paths[group[0]], paths[group[-1]], len(plans[-1]), ragged.MAX_CLIPS))
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for group, plan in zip(groups, plans):
        merge = high_band != "drop" and any(infos[f]["rate"] > SR for f in group)
        if merge or loudness == "source":               # the native planes stay: the merge reads them, 'source' measures them
            ys, _, _ = audio_io.load_channels_batch_device([paths[f] for f in group], sr=None)
            natives = [y[c] for y in ys for c in range(y.shape[0])]
            clips = _to_model_rate(natives, [infos[f]["rate"] for f, y in zip(group, ys) for _ in range(y.shape[0])])
        else:
            ys, _, _ = audio_io.load_channels_batch_device([paths[f] for f in group], sr=SR)
            clips = [y[c] for y in ys for c in range(y.shape[0])]
        owner = [f for f, y in zip(group, ys) for _ in range(y.shape[0])]                           # the file of each channel
        linked = dict(stitch_bits=True, link=owner, link_mode=link_channels) if link_channels is not None else {}
        outs = windows.denoise_long(detector, denoiser, clips, SR, FPS, window_seconds, context_seconds, max_batch, max_columns,
                                    **linked)
        rates = [infos[f]["rate"] for f in owner]
        if merge:
            outs = _merge_back(natives, clips, outs, rates, high_band, smooth_frames)
            rates = [min(r, SR) for r in rates]         # what is left for _resample_back: the rates below SR
        outs = _resample_back(outs, rates)
        per_file, k = {}, 0
        for f, y in zip(group, ys):
            per_file[f] = audio_io.planes_of(outs[k:k + y.shape[0]])
            k += y.shape[0]
        by_format = {}
        for f in group:
            by_format.setdefault(formats[f], []).append(f)
        parts, spans = [], {}
        if loudness is not None:                        # measure what the encode will read, scale it, encode as before
            level = audio_io.planes_together([per_file[f] for f in group])
            per_file.update(zip(group, level))
            frames, rates_g = [infos[f]["frames"] for f in group], [infos[f]["rate"] for f in group]
            w = [weights[f] for f in group]
            measured = {} if limiter is not None else flags        # the limiter's own measurement carries no extra
            if loudness == "source" and not measured:
                got = metrics.loudness_batch(level + list(ys), rates_g * 2, w * 2, frames * 2)
                target = got["rows"].new_empty(len(group)).copy_(got["rows"][len(group):, 0])       # packed, whatever the group's size
            elif loudness == "source":                  # the true peak and the range of the outputs only: the sources apart
                got = metrics.loudness_batch(level, rates_g, w, frames, **measured)
                target = metrics.loudness_batch(list(ys), rates_g, w, frames)["lufs"].contiguous()
            else:
                got = metrics.loudness_batch(level, rates_g, w, frames, **measured)
                target = torch.full((len(group),), float(loudness), dtype=torch.float64, device=got["rows"].device)
            if limiter is not None:                     # the gain to the target in full, the peaks held; then measure what is written
                before = got["rows"][:len(group)].contiguous()
                level, curve = audio_io.limit_batch_device(level, before, target, peak_ceiling_db, rates=rates_g, lookahead_ms=lookahead_ms,
                                                           frames=frames, true_peak=peak == "true")
                per_file.update(zip(group, level))
                got = metrics.loudness_batch(level, rates_g, w, frames, **flags)
            rows = got["rows_true" if peak == "true" else "rows"][:len(group)]               # column 1: the peak the ceiling bounds
            aim = target if limiter is None else got["lufs"].contiguous()    # its own loudness: the gain to it is 1, the trim is left
            gains, limited = audio_io.loudness_gain_batch_device(level, rows, aim, peak_ceiling_db, frames=frames)
            parts += [rows.contiguous().view(torch.uint8).reshape(-1), target.view(torch.uint8),
                      gains.view(torch.uint8), limited.view(torch.uint8)]
            if loudness_range:                          # {LRA, max momentary, max short-term, windows}: windows -1 marks a skipped row
                more = torch.stack([got[k].double() for k in ("lra", "max_momentary", "max_short_term", "windows")], dim=1)
                parts.append(more.contiguous().view(torch.uint8).reshape(-1))
            if limiter is not None:
                parts += [before.view(torch.uint8).reshape(-1), curve.contiguous().view(torch.uint8).reshape(-1)]
        for fmt, files in by_format.items():
            how = dict(dither=dither, seed=int(dither_seed), keys=files) if dither is not None and fmt in audio_io.DITHER_FORMATS else {}
            data, offsets, clipped = audio_io.encode_batch_device([per_file[f] for f in files], fmt,
                                                                  frames=[infos[f]["frames"] for f in files], **how)
            for j, f in enumerate(files):
                spans[f] = (len(parts), int(offsets[j]), int(offsets[j + 1]), j)
            parts += [data, clipped.view(torch.uint8)]
        host = ragged.split(torch.cat(parts).cpu().numpy(), [p.numel() for p in parts])            # the group's one download
        n_windows = np.bincount(plan[:, 0], minlength=len(clips))
        if loudness is not None:
            rows_h, target_h, gains_h, limited_h = host[0].view(np.float64).reshape(-1, 4), host[1].view(np.float64), \
                host[2].view(np.float32), host[3].view(np.bool_)
            if np.any(rows_h[:, 2] < 0):
                raise RuntimeError("sos_loudness_batch_f64: device rows disagree with the host's")
            if peak == "true" and np.any(np.isnan(rows_h[:, 1])):
                raise RuntimeError("sos_true_peak_batch_f64: device rows disagree with the host's")
        if loudness_range:
            more_h = host[4].view(np.float64).reshape(-1, 4)
            if np.any(more_h[:, 3] < 0):
                raise RuntimeError("sos_loudness_range_batch_f64: device rows disagree with the host's")
        if limiter is not None:
            at = 5 if loudness_range else 4
            before_h, curve_h = host[at].view(np.float64).reshape(-1, 4), host[at + 1].view(np.float64).reshape(-1, 4)
            if np.any(before_h[:, 2] < 0) or np.any(curve_h[:, 2] < 0):
                raise RuntimeError("sos_limiter_batch_f32: device rows disagree with the host's")
        for g, f in enumerate(group):
            part, b0, b1, j = spans[f]
            tag, bits = SAMPLE_FORMATS[formats[f]][2:]
            blob = audio_io.wave_container(host[part][b0:b1].tobytes(), tag, infos[f]["channels"], infos[f]["rate"], bits)
            with open(out_paths[f], "wb") as fp:
                fp.write(blob)
            results.append(dict(path=paths[f], out_path=out_paths[f], channels=infos[f]["channels"], rate=infos[f]["rate"],
                                frames=infos[f]["frames"], format=formats[f], clipped=int(host[part + 1].view(np.int64)[j]),
                                windows=int(sum(n_windows[k] for k, o in enumerate(owner) if o == f))))
            if dither is not None:
                results[-1].update(dither=dither if formats[f] in audio_io.DITHER_FORMATS else None)
            if loudness is not None:
                gain_db = after_db = 20.0 * float(np.log10(np.float64(gains_h[g])))           # after_db: what follows the last measurement
                results[-1].update(loudness_before=float(rows_h[g, 0]), loudness=float(rows_h[g, 0]) + gain_db,
                                   loudness_target=float(target_h[g]), gain_db=gain_db, peak_limited=bool(limited_h[g]))
            if limiter is not None:
                gain_db = 20.0 * float(np.log10(curve_h[g, 0])) + after_db
                results[-1].update(loudness_before=float(before_h[g, 0]), gain_db=gain_db, limiter_db=20.0 * float(np.log10(curve_h[g, 1])),
                                   limiter_samples=int(curve_h[g, 2]))
            if peak == "true":
                with np.errstate(divide="ignore"):
                    results[-1].update(true_peak_db=float(20.0 * np.log10(np.float64(gains_h[g]) * rows_h[g, 1])))
            if loudness_range:
                results[-1].update(lra=float(more_h[g, 0]), max_momentary=float(more_h[g, 1]) + after_db,
                                   max_short_term=float(more_h[g, 2]) + after_db)
    return results
