"""Every form of the on-disk hand-off over one seeded fixture, one hash per form (run on the GPU box): what a refactor of
handoff.py is compared with its parent by.  Under --root DIR (which must not exist) it writes
  ds/      five recordings -- 3.2 s (44.1 kHz stereo s16), 2.5 s (framerate 25), 0.8 s, 1.7 s and one of three windows at the
           window and context sizes of tests/test_gpu_handoff_detect_windows.py -- with runs of '0' in their bit streams and
           unlabelled '2' frames at both ends (dataset.json; dataset_plain.json has every frame labelled, which
           create_data_from_prediction needs), and two noise files of 1.5 s (shorter than any crop) and 4 s;
  <precision>/<form>/   what the form wrote, for 'mixed' and 'bf16x3'
and prints per form one line `<precision>/<form> <sha256> <files> <bytes>`: the SHA-256 over the sorted (relative path, bytes)
of the form's tree followed by json.dumps of what the call returned.  The JSONs carry absolute paths, so two runs compare only
under the same --root.  --json FILE also stores the lines.  Nothing is asserted."""
import argparse
import hashlib
import json
import os
import shutil
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sos_amd  # noqa: E402
from oracle import nets as onet  # noqa: E402
from sos_amd import audio_io, handoff, metrics  # noqa: E402
from sos_amd.common import MyConfig  # noqa: E402
from sos_amd.denoiser import networks as jnet  # noqa: E402
from sos_amd.detector import networks as dnet  # noqa: E402

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
N_LONG = 3 * CORE + 5 * HOP + 77
SECONDS = dict(window_seconds=CORE / 14000, context_seconds=CONTEXT / 14000)
# name, stored rate, channels, samples at the stored rate, int16?, framerate
RECORDINGS = [("rec_a", 44100, 2, int(44100 * 3.2), True, 30), ("rec_b", 14000, 1, 35000, False, 25), ("rec_c", 14000, 1, 11200, False, 30),
              ("rec_d", 14000, 1, 23800, False, 30), ("rec_l", 14000, 1, N_LONG, False, 25)]


def _signal(rng, n, sr0):
    t = np.arange(n) / sr0
    env = (np.sin(2 * np.pi * 0.7 * t) > -0.2).astype(np.float64)
    return 0.3 * env * np.sin(2 * np.pi * 220 * t * (1 + 0.3 * np.sin(2 * np.pi * 3 * t))) + 0.05 * rng.standard_normal(n)


def make_fixture(root):
    rng = np.random.default_rng(11)
    files, plain = [], []
    for i, (name, sr0, ch, n, s16, fr) in enumerate(RECORDINGS):
        sig = _signal(rng, n, sr0)
        pcm = np.stack([sig, 0.8 * sig + 0.01 * rng.standard_normal(n)], axis=1)[:, :ch]
        pcm = np.clip(pcm * 32768, -32768, 32767).astype(np.int16) if s16 else pcm.astype(np.float32)
        os.makedirs(os.path.join(root, name))
        with open(os.path.join(root, name, name + "_0000001.wav"), "wb") as fp:
            fp.write(audio_io.wave_bytes(np.ascontiguousarray(pcm if ch > 1 else pcm[:, 0]), sr0))
        secs = n / sr0
        nfr = int(secs * fr)
        bits = "".join("0" if (k // (7 + 2 * i)) % 3 == 1 else "1" for k in range(nfr))
        path = "/authors/machine/ds/%s/%s_0000001.wav" % (name, name)
        entry = dict(path=path, clip_start_time=0, clip_end_time=secs, face_x=0, face_y=0, framerate=fr, audio_sample_rate=sr0,
                     audio_samples=n, duration=secs, num_frames=nfr, bit_stream=bits, silence_total_ratio=0,
                     avg_silenceInterval_silcenceTotal_ratio=0, frames_path=None, flows_path=None, audio_path=path)
        plain.append(entry)
        files.append(dict(entry, bit_stream="2" * (1 + i) + bits[1 + i:-2] + "22"))
    for name, fs in (("dataset.json", files), ("dataset_plain.json", plain)):
        with open(os.path.join(root, name), "w") as fp:
            json.dump(dict(dataset_path="/authors/machine/ds", num_videos=len(fs), files=fs), fp)
    noise = []
    for name, secs in (("noise_short", 1.5), ("noise_long", 4.0)):
        noise.append(os.path.join(root, name + ".wav"))
        audio_io.write_wav(noise[-1], (0.1 * rng.standard_normal(int(14000 * secs))).astype(np.float32), 14000)
    return os.path.join(root, "dataset.json"), os.path.join(root, "dataset_plain.json"), noise


def tree_hash(path, returned):
    h, files, nbytes = hashlib.sha256(), 0, 0
    for d, _, names in sorted(os.walk(path)):
        for name in sorted(names):
            with open(os.path.join(d, name), "rb") as fp:
                data = fp.read()
            rel = os.path.relpath(os.path.join(d, name), path).encode()
            h.update(b"%d:%s:%d:" % (len(rel), rel, len(data)))
            h.update(data)
            files, nbytes = files + 1, nbytes + len(data)
    h.update(json.dumps(returned).encode())
    return h.hexdigest(), files, nbytes


def _detector(shift=0.0):
    sd = onet.closed_form_state(onet.detector_spec(), seed=1)
    sd["fc1.2.bias"] = sd["fc1.2.bias"] - shift
    det = dnet.get_network()
    det.load_state_dict(sd)
    return det.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    os.makedirs(root)
    ds = os.path.join(root, "ds")
    os.makedirs(ds)
    dj, dj_plain, noise = make_fixture(ds)
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    jm = jm.cuda().eval()
    # a detector whose logits on this data set have the median 0, so that both classes occur
    sos_amd.set_precision("bf16x3")
    first = handoff.detect_files(_detector(), dj, os.path.join(root, "probe"), data_root=ds, save_stat=False, batch_files=True)
    conf = np.clip(np.concatenate([np.asarray(it["confidence"], dtype=np.float64) for it in first["data"]]), 1e-6, 1 - 1e-6)
    det = _detector(shift=float(np.median(np.log(conf / (1 - conf)))))
    lines = []

    def form(out, name, fn):
        res = fn(os.path.join(out, name))
        lines.append("%s/%s %s %d %d" % ((os.path.basename(out), name) + tree_hash(os.path.join(out, name), res)))
        print(lines[-1], flush=True)

    for precision in ("mixed", "bf16x3"):
        sos_amd.set_precision(precision)
        out = os.path.join(root, precision)
        # ---- stage 1
        nz = dict(noise_files=noise, snr=3, seed=5)
        for tag, kw in (("", {}), ("_noise", nz)):
            form(out, "s1_file" + tag, lambda o: handoff.detect_files(det, dj, o, data_root=ds, **kw))
            for mb in (64, 2):
                form(out, "s1_batch%d%s" % (mb, tag),
                     lambda o: handoff.detect_files(det, dj, o, data_root=ds, batch_files=True, max_batch=mb, **kw))
        bm = dict(data_root=ds, batch_files=True, batch_mix=True, **nz)
        form(out, "s1_mix", lambda o: handoff.detect_files(det, dj, o, **bm))
        form(out, "s1_mix_two_groups", lambda o: handoff.detect_files(det, dj, o, max_mix_bytes=320000, **bm))
        form(out, "s1_windows", lambda o: handoff.detect_files(det, dj, o, data_root=ds, batch_files=True, **SECONDS))
        form(out, "s1_windows_mix", lambda o: handoff.detect_files(det, dj, o, **bm, **SECONDS))
        # ---- eval_results -> pred_data (every frame labelled); the forms write next to their input, which is copied for each
        src = os.path.join(out, "s1_plain_noise")
        form(out, "s1_plain_noise", lambda o: handoff.detect_files(det, dj_plain, o, data_root=ds, **nz))
        pred = None
        for batch_files in (False, True):
            for clean_audio in (False, True):
                name = "cd_%s_%s" % ("batch" if batch_files else "file", "clean" if clean_audio else "plain")

                def create(o):
                    shutil.copytree(src, o)
                    return handoff.create_data_from_prediction(os.path.join(o, "eval_results_snr3.json"), noise_snr=3, data_root=ds,
                                                               clean_audio=clean_audio, batch_files=batch_files, max_bytes=600000)
                form(out, name, create)
                pred = pred or (os.path.join(out, name, "pred_data_snr3.json") if clean_audio else None)
        # ---- stage 2; pypesq has no counterpart here: a constant stands in.  The per-file measures call stoi_fn, so
        # stoi_fn=True (STOI in the batch's launch sequence) becomes metrics.stoi for that one form
        pesq = lambda c, o, sr: 2.5                                                            # noqa: E731
        for known in (False, True):
            tag = "_known" if known else "_unknown"
            for bmx in (False, True):
                form(out, "s2_files%s%s" % ("_batch_metrics" if bmx else "", tag), lambda o: handoff.denoise_files(
                    jm, handoff.get_data_from_first_model(pred, sr=14000, unknown_clean_signal=not known), o, snr=3,
                    pesq_fn=pesq, stoi_fn=True if bmx else metrics.stoi, batch_metrics=bmx))
            fm = dict(sr=14000, snr=3, unknown_clean_signal=not known, pesq_fn=pesq, stoi_fn=True)
            form(out, "s2_first_model64" + tag, lambda o: handoff.denoise_first_model(jm, pred, o, max_batch=64, **fm))
            form(out, "s2_first_model2" + tag, lambda o: handoff.denoise_first_model(jm, pred, o, max_batch=2, **fm))
            form(out, "s2_first_model_nosave" + tag,
                 lambda o: handoff.denoise_first_model(jm, pred, o, save_individual_results=False, **fm))
            form(out, "s2_first_model_windows" + tag, lambda o: handoff.denoise_first_model(jm, pred, o, **fm, **SECONDS))
    sos_amd.set_precision("bf16")
    if args.json:
        with open(args.json, "w") as fp:
            json.dump(lines, fp, indent=1)


if __name__ == "__main__":
    main()
