"""Denoise WAVE recordings from the command line (recordings.denoise_recordings): every written file keeps its source's frame
count, channels, rate and sample format.

  python tools/denoise_recordings.py DETECTOR.pth DENOISER.pth OUT_DIR in1.wav in2.wav ... [--sample-format s16] [--suffix _dn]
                                     [--link-channels any] [--high-band keep|follow] [--smooth-frames 2]
                                     [--loudness -23|source] [--peak-ceiling-db -1] [--peak sample|true] [--loudness-range]
                                     [--dither tpdf|highpass] [--dither-seed 0] [--limiter lookahead] [--lookahead-ms 5]

The networks run at 14 kHz: by default (--high-band drop) a 44.1 / 48 kHz file comes back band-limited to 7 kHz.  --high-band keep
passes the source's band above 7 kHz through untouched; --high-band follow gives it the attenuation the denoiser applied below.

--loudness brings every written file to a target integrated loudness in LUFS (ITU-R BS.1770 / EBU R128), or with `source` to the
loudness its source had, by one gain per file applied before the samples are quantised; --peak-ceiling-db bounds the sample peak, or with
--peak true the TRUE peak (dBTP, what EBU R128 delivery asks for: 4x interpolation).  --loudness-range also reports the loudness
range (LRA, EBU Tech 3342) and the maximum momentary and short-term loudness of every written file.

--dither adds dither before the 8 / 16 / 24-bit files are rounded (default: plain rounding): tpdf is white, highpass has its
power moved towards half the rate.  What the denoiser left below one LSB then stays signal under a steady noise floor; without it
that residue is distorted or gated to zero.  --dither-seed makes another draw; the same seed writes the same bytes.

--limiter lookahead (with --loudness) holds the peaks at the ceiling by a gain that dips around them only, ramping over twice
--lookahead-ms on either side, so that a file whose peaks would bind the one gain is still written at its target, not below it.

The checkpoints are the reference's (`{clock, model_state_dict, ...}` as the agents save them) or bare state dicts."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sos_amd  # noqa: E402
from sos_amd import audio_io, recordings  # noqa: E402
from sos_amd.common import MyConfig  # noqa: E402
from sos_amd.denoiser import networks as jnet  # noqa: E402
from sos_amd.detector import networks as dnet  # noqa: E402


def _load(net, path):
    ck = torch.load(path, map_location="cpu")
    net.load_state_dict(ck["model_state_dict"] if "model_state_dict" in ck else ck)
    return net.cuda().eval()


def _loudness(text):
    return "source" if text == "source" else float(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("detector", help="checkpoint of the silent-interval detector")
    ap.add_argument("denoiser", help="checkpoint of the denoiser")
    ap.add_argument("out_dir")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--window-seconds", type=float, default=30.0)
    ap.add_argument("--context-seconds", type=float, default=2.0)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--max-columns", type=int, default=65536)
    ap.add_argument("--sample-format", choices=sorted(audio_io.ENCODINGS) + sorted(audio_io.G711), default=None,
                    help="one format for all files, linear PCM / float or G.711 (default: each source's)")
    ap.add_argument("--suffix", default="")
    ap.add_argument("--link-channels", choices=["any", "mean"], default=None,
                    help="the channels of a file share one stream of silent-interval decisions: a frame is speech if ANY channel has "
                         "speech, or if the MEAN logit says so (default: every channel decides on its own)")
    ap.add_argument("--high-band", choices=list(recordings.HIGH_BAND_MODES), default="drop",
                    help="the band above 7 kHz of files above 14 kHz: drop it (default: the output is band-limited to 7 kHz), keep it "
                         "untouched, or let it follow the attenuation the denoiser applied to the low band")
    ap.add_argument("--smooth-frames", type=int, default=2, help="--high-band follow: gains are averaged over 2 K + 1 hop frames (0 .. 16)")
    ap.add_argument("--loudness", type=_loudness, default=None,
                    help="target integrated loudness in LUFS (-70 .. 0), or 'source': the loudness of each file's own source "
                         "(default: the level the networks return)")
    ap.add_argument("--peak-ceiling-db", type=float, default=-1.0, help="--loudness: the peak a levelled file may reach, dBFS / dBTP (<= 0)")
    ap.add_argument("--peak", choices=list(recordings.PEAK_MODES), default="sample",
                    help="--loudness: what --peak-ceiling-db bounds, the sample peak (default) or the true peak (dBTP)")
    ap.add_argument("--loudness-range", action="store_true",
                    help="--loudness: also report the loudness range (LU) and the maximum momentary / short-term loudness (LUFS) of every written file")
    ap.add_argument("--dither", choices=sorted(audio_io.DITHER), default=None,
                    help="dither the files written as u8 / s16 / s24 before rounding: triangular, white (tpdf) or moved towards half the "
                         "rate (highpass) (default: none)")
    ap.add_argument("--dither-seed", type=int, default=0, help="--dither: the seed of the draw, 0 .. 2^64 - 1")
    ap.add_argument("--limiter", choices=list(recordings.LIMITERS), default=None,
                    help="--loudness: hold the peaks at --peak-ceiling-db by a look-ahead limiter and apply the gain to the target in full "
                         "(default: one gain per file, lowered until the peak fits)")
    ap.add_argument("--lookahead-ms", type=float, default=5.0, help="--limiter: the look-ahead, 1 .. 1024 samples at every file's rate")
    ap.add_argument("--precision", default="mixed", choices=["bf16", "bf16x3", "fp16", "mixed"])
    args = ap.parse_args()
    det, jm = _load(dnet.get_network(), args.detector), _load(jnet.get_network(MyConfig()), args.denoiser)
    sos_amd.set_precision(args.precision)
    for r in recordings.denoise_recordings(det, jm, args.files, args.out_dir, args.window_seconds, args.context_seconds, args.max_batch,
                                           args.max_columns, sample_format=args.sample_format, suffix=args.suffix,
                                           link_channels=args.link_channels, high_band=args.high_band,
                                           smooth_frames=args.smooth_frames, loudness=args.loudness,
                                           peak_ceiling_db=args.peak_ceiling_db, peak=args.peak,
                                           loudness_range=args.loudness_range, dither=args.dither, dither_seed=args.dither_seed,
                                           limiter=args.limiter, lookahead_ms=args.lookahead_ms):
        level = "" if args.loudness is None else ", %.2f -> %.2f LUFS (%+.2f dB%s)" % (
            r["loudness_before"], r["loudness"], r["gain_db"], ", peak-limited" if r["peak_limited"] else "")
        if args.limiter is not None:
            level += ", limiter %.2f dB over %d samples" % (r["limiter_db"], r["limiter_samples"])
        if args.peak == "true":
            level += ", %.2f dBTP" % r["true_peak_db"]
        if args.loudness_range:
            level += ", LRA %.2f LU, max M %.2f / S %.2f LUFS" % (r["lra"], r["max_momentary"], r["max_short_term"])
        if r.get("dither"):
            level += ", %s dither" % r["dither"]
        print("%s -> %s: %d x %d frames at %d Hz, %s, %d windows, %d samples clipped%s"
              % (r["path"], r["out_path"], r["channels"], r["frames"], r["rate"], r["format"], r["windows"], r["clipped"], level))


if __name__ == "__main__":
    main()
