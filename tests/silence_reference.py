"""Float64 restatement of the silent-interval labeller (sos_amd.labels, csrc/silence_label.hip) in plain numpy, written from the
contract and not from the kernel.  Test infrastructure, like the oracle.  Parity with the reference's own labeller
(preprocessing/get_bitstream_better) is unpinned: its source is not available; the contract below is this project's.

Per clip x[0..n) (f32 samples), sample rate sr, frame rate fps, ratio = sr / fps in double (> 1):
  frames   F = ceil(n fps / sr); frame i = [int(i ratio), min(int((i+1) ratio), n)), products in double; every frame non-empty.
  energy   E[i] = mean of x^2 over frame i, float64.
  raw      T = max(10^(-threshold_db / 10) max E, floor); quiet[i] = E[i] <= T.
  pass 1   a run of non-quiet frames shorter than min_speech_frames with quiet frames on both sides becomes quiet.
  pass 2   after pass 1, a run of quiet frames shorter than min_silent_frames becomes non-quiet, wherever it lies.
Each pass works over the runs as they were when it began.  bits: 1 = non-silent, 0 = silent.

`undecided` counts the frames with |E - T| <= 4 m u max(E, T), m = the clip's longest frame in samples, u = 2^-53: the terms
of the sums are non-negative, so any summation order is within (m - 1) u relative of the exact sum, and T carries one more such
error; a frame outside that band gets the same raw decision from every correctly rounded implementation."""
import math
from itertools import groupby

import numpy as np

U = 2.0 ** -53
RATES = [(14000, 30.0), (44100, 30.0), (16000, 29.97), (8000, 25.0), (14000, 30000 / 1001)]
LOUD, QUIET = 0.3, 3e-4            # plan clips: |sample| of a loud / a quiet frame; the energies are 9e-2 and 9e-8


def frame_count(n, sr, fps):
    return int(math.ceil(n * fps / sr))


def frame_edges(n, sr, fps, frames=None):
    """(lo, hi) int arrays of the frames' sample ranges."""
    ratio = sr / fps
    F = frame_count(n, sr, fps) if frames is None else frames
    lo = np.array([min(int(i * ratio), n) for i in range(F)], dtype=np.int64)
    hi = np.array([min(int((i + 1) * ratio), n) for i in range(F)], dtype=np.int64)
    return lo, hi


def seconds_to_frames(seconds, fps):
    return max(1, int(round(seconds * fps)))


def run_passes(quiet, min_silent_frames=1, min_speech_frames=1):
    """The two run-length passes over a 0/1 sequence (1 = quiet) -> the final quiet sequence."""
    q = np.asarray(quiet, dtype=np.int64)
    runs = [(k, len(list(g))) for k, g in groupby(q.tolist())]
    one, pos = q.copy(), 0
    for j, (k, length) in enumerate(runs):
        if k == 0 and length < min_speech_frames and 0 < j < len(runs) - 1:
            one[pos:pos + length] = 1
        pos += length
    two, pos = one.copy(), 0
    for k, g in groupby(one.tolist()):
        length = len(list(g))
        if k == 1 and length < min_silent_frames:
            two[pos:pos + length] = 0
        pos += length
    return two


def label(x, sr, fps=30.0, threshold_db=40.0, min_silent_frames=1, min_speech_frames=1, floor=0.0):
    """-> dict(bits uint8 (1 = non-silent), energy f64, max_energy, threshold, silent_frames, silent_runs, frames, longest,
    undecided)."""
    x = np.asarray(x)
    n = len(x)
    if n < 1 or not sr / fps > 1.0:
        raise ValueError("an empty clip, or no more than one sample per frame")
    lo, hi = frame_edges(n, sr, fps)
    if not (np.all(hi > lo) and hi[-1] == n and lo[0] == 0 and np.all(lo[1:] == hi[:-1])):
        raise AssertionError(f"the frames do not tile the clip: n={n} sr={sr} fps={fps}")
    sq = x.astype(np.longdouble) ** 2                          # 64-bit significands: the sums' error is far below u
    E = (np.add.reduceat(sq, lo) / (hi - lo)).astype(np.float64)
    T = max(10.0 ** (-threshold_db / 10.0) * float(E.max()), floor)
    m = int((hi - lo).max())
    undecided = int(np.sum(np.abs(E - T) <= 4 * m * U * np.maximum(E, T)))
    quiet = run_passes((E <= T).astype(np.int64), min_silent_frames, min_speech_frames)
    silent_runs = sum(1 for k, _ in groupby(quiet.tolist()) if k == 1)
    return dict(bits=(1 - quiet).astype(np.uint8), energy=E, max_energy=float(E.max()), threshold=T,
                silent_frames=int(quiet.sum()), silent_runs=silent_runs, frames=len(E), longest=m, undecided=undecided)


def label_seconds(x, sr, fps=30.0, threshold_db=40.0, min_silence=0.1, min_speech=0.0, floor=0.0):
    """label() with the Python layer's arguments: the minimum lengths in seconds."""
    return label(x, sr, fps, threshold_db, seconds_to_frames(min_silence, fps), seconds_to_frames(min_speech, fps), floor)


# ---- generators shared by tests/test_silence_reference.py (which asserts undecided == 0 for them) and tests/test_gpu_labels.py
def plan_from_string(s):
    """'1' = a loud frame, '0' = a quiet one (the bits a labeller without run rules gives); blanks are ignored."""
    return np.array([int(c) for c in s if c in "01"], dtype=np.uint8)


def plan_samples(plan, sr, fps, seed=0, last_frame_samples=None):
    """A clip whose frame i holds +-LOUD (plan[i] = 1) or +-QUIET (plan[i] = 0) at random signs, so that its energy is the
    square of that value whatever the frame's length.  The clip is the longest one with len(plan) frames, or ends
    last_frame_samples into its last frame."""
    plan = np.asarray(plan)
    F, ratio = len(plan), sr / fps
    start = int((F - 1) * ratio)
    n = int(F * ratio) if last_frame_samples is None else start + last_frame_samples
    while frame_count(n, sr, fps) > F:          # (the rounding of n fps / sr at a whole number of frames)
        n -= 1
    assert n > start and frame_count(n, sr, fps) == F, (n, sr, fps, F)
    lo, hi = frame_edges(n, sr, fps)
    rng = np.random.default_rng(seed)
    x = np.where(rng.integers(0, 2, size=n) == 1, 1.0, -1.0).astype(np.float32)
    for i in range(F):
        x[lo[i]:hi[i]] *= np.float32(LOUD if plan[i] else QUIET)
    return x


MIN_FRAMES = 4                     # the minimum run length (frames) of the tile cases, for both passes


def tile_cases(sr, fps):
    """[(name, plan)] around the 256-frame scan tile of the label kernel, for minimum run lengths of MIN_FRAMES frames: random
    plans of 1, 2, 255, 256, 257 and 513 frames; in 257 and 513 frames a quiet run among loud frames, and a loud run among quiet
    ones, of MIN_FRAMES - 1, MIN_FRAMES and MIN_FRAMES + 1 frames beginning at frame 250, and one whose last frame is 255 and
    one whose last frame is 256."""
    rng = np.random.default_rng([int(sr), int(fps * 1000)])
    cases = []
    for F in (1, 2, 255, 256, 257, 513):
        plan = np.repeat(rng.integers(0, 2, size=F), rng.integers(1, 2 * MIN_FRAMES, size=F))[:F].astype(np.uint8)
        plan[int(rng.integers(0, F))] = 1                       # at least one loud frame: the threshold follows it
        cases.append((f"random{F}", plan))
        if F < 257:
            continue
        spans = [(250, 250 + d) for d in (MIN_FRAMES - 1, MIN_FRAMES, MIN_FRAMES + 1)] + [(250, 256), (250, 257)]
        for a, b in spans:
            for run in (0, 1):                                  # a quiet run among loud frames, a loud run among quiet ones
                plan = np.full(F, 1 - run, dtype=np.uint8)
                plan[a:b] = run
                if run == 1 and b - a >= MIN_FRAMES:
                    plan[:8] = 1                                # a second loud run, at the clip's start
                cases.append((f"{'loud' if run else 'quiet'}{a}to{b}of{F}", plan))
    return cases


def speechlike(seed, seconds, sr):
    """Amplitude-modulated noise: bursts of 0.1 .. 0.6 s at levels over 50 dB with quiet gaps between them."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    env = np.zeros(n)
    pos = 0
    while pos < n:
        length = int(rng.uniform(0.1, 0.6) * sr)
        level = 10.0 ** (-rng.uniform(0.0, 50.0) / 20.0) if rng.random() < 0.6 else 10.0 ** (-rng.uniform(55.0, 80.0) / 20.0)
        env[pos:pos + length] = level
        pos += length
    return (0.5 * env * rng.standard_normal(n)).astype(np.float32)


def speech_cases():
    """[(x, sr, fps)]: ten clips of about 3 s at the rates of RATES, two each."""
    return [(speechlike(900 + i, 2.6 + 0.1 * i, RATES[i % 5][0]),) + RATES[i % 5] for i in range(10)]


def batch_cases():
    """[(x, sr, fps)]: twelve ragged clips of 0.2 .. 2.4 s (odd lengths, so that the clips start at every alignment)."""
    return [(speechlike(700 + i, 0.2 + 0.2 * i + 0.0007 * (i + 1), RATES[i % 5][0]),) + RATES[i % 5] for i in range(12)]
