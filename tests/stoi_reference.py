"""Float64 numpy/scipy restatement of STOI (Taal et al., IEEE TASLP 19(7), 2011) and extended STOI (Jensen & Taal,
IEEE/ACM TASLP 24(11), 2016) with pystoi's interface `stoi(x, y, fs_sig, extended=False)` (x = clean, y = processed).
Test infrastructure, like tests/lstm_reference.py: the oracle of sos_amd.metrics.stoi / stoi_batch.

Choices this restatement makes where pystoi versions differ (parity against pystoi itself is unpinned, the package is
not available to the test suite):
* frame loops (silent-frame removal and STFT) start frames at 0, 128, ... while the start is < len - 256, the bound
  of the Matlab original;
* ESTOI leaves out pystoi's EPS-scale random dither before the row / column normalisations (the result is
  deterministic; the difference is below 1e-12) and divides by (norm + EPS), as classic STOI does;
* a clip with no complete 256-sample frame at 10 kHz (pystoi fails inside numpy there) is treated like any clip with
  fewer than 30 STFT frames: a RuntimeWarning and 1e-5."""
import math
import warnings

import numpy as np

FS = 10000
N_FRAME = 256
HOP = N_FRAME // 2
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.
DYN_RANGE = 40
EPS = np.finfo(float).eps
WINDOW = np.hanning(N_FRAME + 2)[1:-1]


def thirdoct(fs=FS, nfft=NFFT, num_bands=NUMBAND, min_freq=MINFREQ):
    """(obm [num_bands][nfft/2+1], centre frequencies, bin ranges [(lo, hi)]): band k sums bins [lo_k, hi_k), the
    edges min_freq 2^((2k -+ 1)/6) snapped to the nearest bin (pystoi's utils.thirdoct)."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands).astype(float)
    cf = np.power(2. ** (1. / 3), k) * min_freq
    lo = min_freq * np.power(2., (2 * k - 1) / 6)
    hi = min_freq * np.power(2., (2 * k + 1) / 6)
    obm = np.zeros((num_bands, len(f)))
    ranges = []
    for i in range(num_bands):
        a = int(np.argmin(np.square(f - lo[i])))
        b = int(np.argmin(np.square(f - hi[i])))
        obm[i, a:b] = 1
        ranges.append((a, b))
    return obm, cf, ranges


OBM, CF, BAND_RANGES = thirdoct()


def resample_ratio(fs_sig):
    """(p, q): 10 kHz / fs_sig reduced by the gcd."""
    g = math.gcd(FS, int(fs_sig))
    return FS // g, int(fs_sig) // g


def resample_taps(fs_sig):
    """Octave's resample filter as pystoi's _resample_window_oct builds it, normalised to unit sum:
    fc = 1/(2 max(p,q)), roll-off fc/10, 60 dB rejection, Kaiser beta = 0.1102 (60 - 8.7)."""
    p, q = resample_ratio(fs_sig)
    fc = 1. / (2 * max(p, q))
    roll = fc / 10
    rej = 60.
    L = int(np.ceil((rej - 8) / (28.714 * roll)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (rej - 8.7)) * (2 * p * fc * np.sinc(2 * fc * t))
    return h / h.sum()


def resample_oct(x, fs_sig):
    """scipy.signal.resample_poly(x, p, q, window=resample_taps(fs_sig)) written out as the polyphase sum the kernel
    computes: y[m] = p sum_i x[i] h[L + m q - i p] over the taps inside h, ceil(n p / q) outputs."""
    x = np.asarray(x, dtype=np.float64)
    p, q = resample_ratio(fs_sig)
    if p == q:
        return x.copy()
    h = resample_taps(fs_sig) * p
    L = (len(h) - 1) // 2
    n = len(x)
    n_out = -(-n * p // q)
    y = np.zeros(n_out)
    T = -(-(2 * L + 1) // p) + 1
    for m0 in range(0, n_out, 1024):
        m = np.arange(m0, min(n_out, m0 + 1024))[:, None]
        i = -((L - m * q) // p) + np.arange(T)[None, :]          # ceil((m q - L) / p) + j
        hi = L + m * q - i * p
        ok = (hi >= 0) & (i >= 0) & (i < n)
        y[m0:m0 + len(m)] = np.sum(np.where(ok, x[np.clip(i, 0, n - 1)] * h[np.clip(hi, 0, 2 * L)], 0.), axis=1)
    return y


def frame_starts(n):
    return np.arange(0, n - N_FRAME, HOP)


def frames(x, starts):
    """[len(starts)][256] windowed frames."""
    return WINDOW * x[np.asarray(starts, dtype=np.int64)[:, None] + np.arange(N_FRAME)[None, :]]


def frame_energies(x):
    """20 log10(||w x_frame|| + EPS) of every frame (dB)."""
    return 20 * np.log10(np.linalg.norm(frames(x, frame_starts(len(x))), axis=1) + EPS)


def keep_mask(x):
    """(mask of the frames that stay, smallest |energy - threshold| in dB)."""
    e = frame_energies(x)
    if len(e) == 0:
        return np.zeros(0, bool), np.inf
    d = np.max(e) - DYN_RANGE - e
    return d < 0, float(np.min(np.abs(d)))


def _overlap_add(fr):
    K = len(fr)
    out = np.zeros((K - 1) * HOP + N_FRAME) if K else np.zeros(0)
    for k in range(K):
        out[k * HOP:k * HOP + N_FRAME] += fr[k]
    return out


def remove_silent_frames(x, y):
    mask, _ = keep_mask(x)
    st = frame_starts(len(x))[mask]
    return _overlap_add(frames(x, st)), _overlap_add(frames(y, st))


def stft(x):
    """rfft (n = 512) of the windowed frames, [frames][257]."""
    return np.fft.rfft(frames(x, frame_starts(len(x))), n=NFFT, axis=1)


def _normalize(v, axis):
    v = v - np.mean(v, axis=axis, keepdims=True)
    return v / (np.linalg.norm(v, axis=axis, keepdims=True) + EPS)


def analyse(x, y, fs_sig, extended=False):
    """dict(score, kept_frames, stft_frames, margin_db) of one clip; score is 1e-5 (with a RuntimeWarning) when fewer
    than 30 STFT frames remain."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError(f"x and y should have the same length, found {x.shape} and {y.shape}")
    if fs_sig != FS:
        x, y = resample_oct(x, fs_sig), resample_oct(y, fs_sig)
    mask, margin = keep_mask(x)
    x, y = remove_silent_frames(x, y)
    xs, ys = stft(x), stft(y)
    res = dict(kept_frames=int(mask.sum()), stft_frames=len(xs), margin_db=margin)
    if len(xs) < N:
        warnings.warn("Not enough STFT frames to compute intermediate intelligibility measure after removing silent "
                      "frames. Returning 1e-5. Please check you wav files", RuntimeWarning)
        res["score"] = 1e-5
        return res
    x_tob = np.sqrt(OBM @ np.square(np.abs(xs.T)))
    y_tob = np.sqrt(OBM @ np.square(np.abs(ys.T)))
    xseg = np.array([x_tob[:, m - N:m] for m in range(N, x_tob.shape[1] + 1)])
    yseg = np.array([y_tob[:, m - N:m] for m in range(N, y_tob.shape[1] + 1)])
    if extended:
        xn = _normalize(_normalize(xseg, 2), 1)
        yn = _normalize(_normalize(yseg, 2), 1)
        res["score"] = float(np.sum(xn * yn / N) / xn.shape[0])
    else:
        norm = np.linalg.norm(xseg, axis=2, keepdims=True) / (np.linalg.norm(yseg, axis=2, keepdims=True) + EPS)
        yp = np.minimum(yseg * norm, xseg * (1 + 10 ** (-BETA / 20)))
        res["score"] = float(np.sum(_normalize(yp, 2) * _normalize(xseg, 2)) / (xseg.shape[0] * xseg.shape[1]))
    return res


def stoi(x, y, fs_sig, extended=False):
    return analyse(x, y, fs_sig, extended)["score"]


def closed_form_pair(idx, n, sr, noise):
    """(clean, processed) f32 test clip: the tests/test_metrics.py::signals speech-like clean signal (on/off envelope,
    frequency-modulated 210 Hz tone, 1.9 kHz tone, low hashed noise floor) and the clean signal plus `noise` times hashed
    white noise."""
    from util import hashed
    t = np.arange(n) / sr
    env = (np.sin(2 * np.pi * 0.9 * t + 0.4) > -0.3).astype(np.float64)
    clean = env * (0.3 * np.sin(2 * np.pi * 210 * t * (1 + 0.2 * np.sin(2 * np.pi * 2.5 * t))) + 0.1 * np.sin(2 * np.pi * 1900 * t))
    clean = clean + 0.002 * hashed(idx, (n,))
    return clean.astype(np.float32), (clean + noise * hashed(idx + 1, (n,))).astype(np.float32)
