"""Float64 restatement of sos_ragged_mix_f32 (csrc/ragged_mix.hip; sos_amd.tools.add_signals_ragged) and the inputs its tests
share.  Per clip: the sample mask of the frame decisions (oracle.frontend.convert_bitstreammask_to_audiomask), the zero-filled
noise crop of handoff.add_noise_to_audio, then add_signals with one noise (oracle.frontend.add_signals, M2/tools.py:217-276)
written out: energies, gain, peak, the three outputs.  Test infrastructure like the oracle; numpy only."""
import numpy as np

from oracle import frontend as ofe

TINY = 1e-30                        # stands for the peak of an all-zero output in the relative bounds
OUT_TOL = 6e-7                      # |got - ref| <= OUT_TOL max(peak of the reference's mixed, TINY): four f32 roundings
MAX_SPREAD = 2.0                    # a fixture's clean and scaled noise stay within twice the peak of their sum (`spread` of mix)
FACTOR_TOL = 2.0 ** -23             # gain, inv: one f32 rounding plus the energies' error
SNRS = (-10.0, 0.0, 7.0)


def crop(noise_len, start, count, n):
    """(first sample, valid samples) of noise[start : start + count] clipped to the recording and to a clip of n samples."""
    nz = max(0, min(int(count), int(n), int(noise_len) - int(start)))
    return (int(start) if nz else 0), nz


def mix(clip, noise, snr, start=0, count=None, bits=None, ratio=None, norm=0.5):
    """dict(mixed, clean, noise, mask, Es, Ez, gain, peak, inv, spread) of one clip in float64.  spread = the larger of
    max |clean| and max |noise| over max |mixed| (0 for an all-zero mix): how far the two terms cancel in their sum.  The f32
    roundings of the kernel are relative to the term they act on, so OUT_TOL, a bound relative to the peak of the SUM, stands
    for four roundings of 2^-24 on terms of at most MAX_SPREAD peaks: 4 x 2 x 6e-8 = 4.8e-7."""
    x = np.asarray(clip, dtype=np.float64)
    n = len(x)
    mask = np.zeros(n, dtype=np.float64)
    if bits is not None:
        mask = ofe.convert_bitstreammask_to_audiomask(x, float(ratio), [int(b) for b in bits])
    s = x * (1.0 - mask)
    noff, nz = crop(len(noise), start, n if count is None else count, n)
    z = np.zeros(n, dtype=np.float64)
    z[:nz] = np.asarray(noise, dtype=np.float64)[noff:noff + nz]
    Es, Ez = float(np.sum(s * s)), float(np.sum(z * z))
    gain = 1.0 if Es == 0.0 or Ez == 0.0 else float(np.sqrt(Es / np.power(10.0, snr / 10.0)) / np.sqrt(Ez))
    m = s + gain * z
    peak = float(np.max(np.abs(m)))
    inv = float(norm) / peak if norm and peak != 0.0 else 1.0
    spread = max(float(np.max(np.abs(s))), float(np.max(np.abs(gain * z)))) / peak if peak != 0.0 else 0.0
    return dict(mixed=m * inv, clean=s * inv, noise=gain * z * inv, mask=mask, Es=Es, Ez=Ez, gain=gain, peak=peak, inv=inv,
                spread=spread)


# ------------------------------------------------------------------------------------------------- shared inputs
def edge_lengths(C):
    """Clips around the 4-sample vector and the chunk of C samples; back to back most start off a 16-byte boundary."""
    return [1, 2, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, 3 * C]


def edge_case(C, seed=35):
    """(clips, recording, snrs, starts): clip i of edge_lengths(C) takes its noise from offset i of ONE recording, so the crops
    overlap and are unaligned; the SNRs cycle through SNRS.  (The seed is one under which no clip's two terms cancel beyond
    MAX_SPREAD: with two samples at 0 dB they easily do -- seed 31 gave a spread of 35 -- and tests/test_mix_reference.py asserts
    the spread of every fixture.)"""
    rng = np.random.default_rng(seed)
    lens = edge_lengths(C)
    clips = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    recording = (0.1 * rng.standard_normal(3 * C + len(lens))).astype(np.float32)
    return clips, recording, [SNRS[i % 3] for i in range(len(lens))], list(range(len(lens)))


def speech_case(seed=9):
    """(clips, noises, snrs, bits, ratios) at 14 kHz: the speech-like generator of tests/test_gpu_handoff_files_batch._fixture
    for 2.0, 1.3, 1.7 and 0.8 s, frame decisions at 30, 25 and 30 frames per second and one clip without any."""
    rng = np.random.default_rng(seed)
    clips, noises, bits, ratios = [], [], [], []
    for k, (secs, fps) in enumerate(((2.0, 30), (1.3, 25), (1.7, None), (0.8, 30))):
        n = int(14000 * secs)
        t = np.arange(n) / 14000
        clips.append((0.3 * np.sin(2 * np.pi * 300 * t) * (0.2 + (np.sin(2 * np.pi * 1.3 * t) > -0.4))
                      + 0.003 * rng.standard_normal(n)).astype(np.float32))
        noises.append((0.05 * rng.standard_normal(n + 100 * k)).astype(np.float32))
        if fps is None:
            bits.append(None)
            ratios.append(None)
        else:
            nfr = int(round(fps * secs))
            bits.append(np.asarray([0 if (i // 7) % 4 == 1 else 1 for i in range(nfr)], dtype=np.uint8))
            ratios.append(14000.0 / fps)
    return clips, noises, [SNRS[k % 3] for k in range(4)], bits, ratios


def silenced_case(seed=12):
    """(clip, noise, bits, ratio): every frame decision silent at 14 kHz / 30 fps over exactly 20 frames -- the oracle's mask
    is 1 on every sample (tests/test_mix_reference.py asserts it), so the signal that is mixed is all zero."""
    rng = np.random.default_rng(seed)
    n = int(20 * 14000 / 30.0)
    return ((0.3 * rng.standard_normal(n)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32),
            np.zeros(20, dtype=np.uint8), 14000 / 30.0)
