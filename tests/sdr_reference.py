"""Float64 numpy/scipy restatement of the two distortion measures of sos_amd.metrics (csrc/sdr.hip), x = clean
(reference) and y = estimate, equal lengths.  Test infrastructure, like tests/stoi_reference.py.

* SI-SDR: oracle/frontend.py::si_sdr(est=y, ref=x), optionally on mean-removed signals.
* SDR: BSS-eval v3 with one source (Vincent et al., IEEE TASLP 14(4), 2006; mir_eval.separation.bss_eval_sources): the
  estimate is projected on the span of the L = filter_length delayed copies of the clean signal; with
  r[k] = sum_t x[t] x[t+k], d[k] = sum_t x[t] y[t+k] (k < L, terms past the end zero), G = toeplitz(r), c = G^-1 d,
  p = d.c and e = sum y^2:  SDR = 10 log10(p / (e - p)).  `sdr_explicit` is mir_eval's own decomposition (signals padded
  to n + L - 1, s_target + e_spat = the projection, e_artif = the rest); the projection is orthogonal, so both agree.
  Parity against mir_eval itself is unpinned (the package is not available to the test suite)."""
import numpy as np
import scipy.linalg
import scipy.signal

from oracle import frontend as ofe

FILTER_LENGTH = 512


def _f64(x, y):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError(f"x and y should have the same length, found {x.shape} and {y.shape}")
    return x, y


def correlations(x, y, L=FILTER_LENGTH):
    """(r, d, e): r[k] = sum_t x[t] x[t+k], d[k] = sum_t x[t] y[t+k] for k < L as direct sums, e = sum y^2."""
    x, y = _f64(x, y)
    n = len(x)
    r, d = np.zeros(L), np.zeros(L)
    for k in range(min(L, n)):
        r[k] = np.dot(x[:n - k], x[k:])
        d[k] = np.dot(x[:n - k], y[k:])
    return r, d, float(np.dot(y, y))


def _db(p, e):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10 * np.log10(p / (e - p))) if e - p > 0 else float("inf")


def sdr(x, y, L=FILTER_LENGTH):
    r, d, e = correlations(x, y, L)
    c = np.linalg.solve(scipy.linalg.toeplitz(r), d)
    return _db(float(d @ c), e)


def levinson(r, d):
    """c with toeplitz(r) c = d by the Levinson-Durbin recursion for a general right-hand side, plain float64, in the
    order the kernel runs it; (c, ok) with ok False when r[0] == 0 or the prediction error stops being positive."""
    L = len(r)
    c, a = np.zeros(L), np.zeros(L)            # a[1..m]: order-m forward predictor
    if not r[0] > 0:
        return c, False
    E = r[0]
    c[0] = d[0] / E
    for m in range(1, L):
        k = -(r[m] + np.dot(a[1:m], r[m - 1:0:-1])) / E
        qn = d[m] - np.dot(c[:m], r[m:0:-1])
        a[1:m] = a[1:m] + k * a[m - 1:0:-1]
        a[m] = k
        E = E * (1 - k * k)
        if not E > 0:
            return c, False
        q = qn / E
        c[:m] = c[:m] + q * a[m:0:-1]
        c[m] = q
    return c, True


def sdr_levinson(x, y, L=FILTER_LENGTH):
    r, d, e = correlations(x, y, L)
    c, ok = levinson(r, d)
    return _db(float(d @ c), e) if ok else float("nan")


def sdr_explicit(x, y, L=FILTER_LENGTH):
    """mir_eval's decomposition written out: the projection of the zero-padded estimate on the L delayed copies of the
    zero-padded clean signal, then ||s_true + e_spat||^2 / ||e_artif||^2."""
    x, y = _f64(x, y)
    n = len(x)
    xp, yp = np.concatenate([x, np.zeros(L - 1)]), np.concatenate([y, np.zeros(L - 1)])
    nfft = int(2 ** np.ceil(np.log2(n + L - 1)))
    X, Y = np.fft.rfft(xp, nfft), np.fft.rfft(yp, nfft)
    r = np.fft.irfft(np.abs(X) ** 2, nfft)[:L]
    d = np.fft.irfft(np.conj(X) * Y, nfft)[:L]
    c = np.linalg.solve(scipy.linalg.toeplitz(r), d)
    proj = scipy.signal.fftconvolve(xp, c)[:n + L - 1]           # s_true + e_spat
    e_artif = yp - proj
    return float(10 * np.log10(np.dot(proj, proj) / np.dot(e_artif, e_artif)))


def si_sdr(x, y, zero_mean=False):
    x, y = _f64(x, y)
    if zero_mean:
        x, y = x - np.mean(x), y - np.mean(y)
    return float(ofe.si_sdr(y, x))


def analyse(x, y, L=FILTER_LENGTH):
    """dict(score, p, e, r0, cond, one_minus_p_over_e, lu_minus_levinson_db) of one clip."""
    r, d, e = correlations(x, y, L)
    G = scipy.linalg.toeplitz(r)
    c = np.linalg.solve(G, d)
    p = float(d @ c)
    score = _db(p, e)
    cl, ok = levinson(r, d)
    lev = _db(float(d @ cl), e) if ok else float("nan")
    both_inf = np.isinf(score) and np.isinf(lev)
    return dict(score=score, p=p, e=e, r0=float(r[0]), cond=float(np.linalg.cond(G)), one_minus_p_over_e=1 - p / e,
                lu_minus_levinson_db=0.0 if both_inf else abs(score - lev))


def filtered_pair(idx, n, sr, noise=0.05):
    """(clean, estimate): the closed-form clean clip through a 200-tap filter with taps at 0, 37 and 150, plus hashed
    white noise: far from the clean signal at lag 0 (low SI-SDR), inside the 512-tap span (high SDR)."""
    from stoi_reference import closed_form_pair
    from util import hashed
    x, _ = closed_form_pair(idx, n, sr, 0.0)
    h = np.zeros(200)
    h[0], h[37], h[150] = 0.6, -0.5, 0.4
    y = np.convolve(x.astype(np.float64), h)[:n] + noise * 0.1 * hashed(idx + 1, (n,))
    return x, y.astype(np.float32)


def lowpassed_pair(idx, n, sr, noise=0.05):
    """(clean, estimate) with the clean clip through an 8th-order Butterworth low-pass at 3.4 kHz (sr = 16000: its lag
    matrix is ill-conditioned, cond(G) about 1e13), estimate = clean + hashed white noise."""
    from stoi_reference import closed_form_pair
    from util import hashed
    x, _ = closed_form_pair(idx, n, sr, 0.0)
    sos = scipy.signal.butter(8, 3400.0, btype="low", fs=sr, output="sos")
    x = scipy.signal.sosfilt(sos, x.astype(np.float64)).astype(np.float32)
    return x, (x.astype(np.float64) + noise * hashed(idx + 1, (n,))).astype(np.float32)


# the five closed-form clips the definitions were checked on: (idx, fs, seconds, noise, SDR in dB at L = 512)
TABLE = [(21, 16000, 2.0, 0.05, 15.654056), (22, 16000, 5.0, 0.3, 0.354973), (23, 16000, 1.0, 0.002, 43.290887),
         (24, 8000, 3.3, 0.1, 9.542270), (25, 16000, 10.0, 0.5, -4.366034)]


def table_pair(row):
    from stoi_reference import closed_form_pair
    idx, fs, seconds, noise, _ = row
    return closed_form_pair(idx, int(seconds * fs), fs, noise)
