"""Host-only checks of the general STFT / ISTFT geometries (no GPU): the oracle against torch.stft / torch.istft in
float64, the packed MFMA matrices of csrc/stft_mfma.hip unpacked into dense float64 matrices against the oracle, the
reference geometry's packed bytes pinned, and the refused geometries."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import frontend as ofe

# (n_fft, hop, win): the geometry set of tests/test_gpu_frontend_geometry.py
GEOMS = [(512, 128, 512), (400, 160, 400), (510, 128, 400), (256, 64, 256), (1024, 256, 1024), (2048, 512, 2048),
         (2048, 128, 2048), (512, 128, 301), (882, 441, 882), (510, 157, 400), (256, 256, 256), (256, 200, 160),
         (16, 4, 16)]
# torch.istft refuses a window envelope with zeros: no overlap with w[0] = 0 (256/256/256) and hop > win leave gaps
NOLA = [g for g in GEOMS if g not in ((256, 256, 256), (256, 200, 160))]
# (n_fft, hop, win, words of the message)
REFUSED = [(511, 128, 511, "n_fft must be even"), (512, 128, 513, "win_length must be in"),
           (512, 128, 15, "win_length must be in"), (512, 0, 512, "hop_length must be in"),
           (512, 513, 512, "hop_length must be in"), (2048, 127, 2048, "ceil(win_length/hop_length) must be <= 16"),
           (4096, 1024, 4096, "n_fft must be in [16, 2048]")]

FE_SD, FE_IE = 16.0, 4096.0        # the power-of-two scales folded into the packed D / E (csrc/stft_mfma.hip)


def _clip(n_fft, hop, seed):
    n = max(4 * n_fft, 12 * hop) + 37
    return np.random.default_rng(seed).standard_normal(n) * 0.1


def _torch_window(win):
    return torch.hann_window(win, periodic=True, dtype=torch.float64)


@pytest.mark.parametrize("n_fft,hop,win", GEOMS)
def test_oracle_stft_matches_torch(n_fft, hop, win):
    x = _clip(n_fft, hop, 1)
    S = ofe.stft_complex(x, n_fft, hop, win)
    R = torch.stft(torch.from_numpy(x), n_fft, hop, win, window=_torch_window(win), center=True, pad_mode="reflect",
                   return_complex=True).numpy()
    assert S.shape == R.shape == (n_fft // 2 + 1, 1 + len(x) // hop)
    assert np.max(np.abs(S - R)) <= 1e-6 * np.max(np.abs(R))


@pytest.mark.parametrize("n_fft,hop,win", NOLA)
def test_oracle_istft_matches_torch(n_fft, hop, win):
    rng = np.random.default_rng(2)
    T = 12
    S = rng.standard_normal((n_fft // 2 + 1, T)) + 1j * rng.standard_normal((n_fft // 2 + 1, T))
    y = ofe.istft_complex(S, hop, win)
    r = torch.istft(torch.from_numpy(S), n_fft, hop, win, window=_torch_window(win), center=True).numpy()
    assert y.shape == r.shape == (hop * (T - 1),)
    assert np.max(np.abs(y - r)) <= 1e-6 * np.max(np.abs(r))


def _lib():
    from sos_amd import _lib
    return _lib.lib()


def _unpack(hi, lo, rtiles, ksteps, scale):
    """[(ks*rtiles + rt)*64 + lane][e] = M[rt*32 + (lane&31)][ks*16 + 8*(lane>>5) + e] -> dense f64 (hi + lo) / scale."""
    v = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)
    v = v.reshape(ksteps, rtiles, 2, 32, 8)                     # ks, rt, lane>>5, lane&31, e
    return v.transpose(1, 3, 0, 2, 4).reshape(rtiles * 32, ksteps * 16) / scale


def _pack_stft(n_fft, hop, win):
    h = _lib()
    nb = h.sos_stft_matrix_bytes(n_fft, hop, win)
    assert nb > 0
    hi, lo = np.full(nb // 2, 0xFFFF, np.uint16), np.full(nb // 2, 0xFFFF, np.uint16)
    assert h.sos_stft_pack_matrix(n_fft, hop, win, hi.ctypes.data, lo.ctypes.data) == 0
    return nb, hi, lo


def _pack_istft(n_fft, hop, win):
    h = _lib()
    nb = h.sos_istft_matrix_bytes(n_fft, hop, win)
    assert nb > 0
    hi, lo = np.full(nb // 2, 0xFFFF, np.uint16), np.full(nb // 2, 0xFFFF, np.uint16)
    wsq = np.full(win, np.nan, np.float32)
    assert h.sos_istft_pack_matrix(n_fft, hop, win, hi.ctypes.data, lo.ctypes.data, wsq.ctypes.data) == 0
    return nb, hi, lo, wsq


@pytest.mark.parametrize("n_fft,hop,win", GEOMS)
def test_stft_packed_matrix_is_the_windowed_dft(n_fft, hop, win):
    nbins = n_fft // 2 + 1
    rtiles, ksteps = -(-2 * nbins // 32), -(-win // 16)
    nb, hi, lo = _pack_stft(n_fft, hop, win)
    assert nb == ksteps * rtiles * 64 * 16
    D = _unpack(hi, lo, rtiles, ksteps, FE_SD)
    assert not D[2 * nbins:].any() and not D[:, win:].any(), "padding rows / columns must be exactly zero"
    x = _clip(n_fft, hop, 3)
    xp = np.pad(x, n_fft // 2, mode="reflect")
    T = 1 + len(x) // hop
    lpad = (n_fft - win) // 2
    frames = xp[lpad + np.arange(win)[:, None] + hop * np.arange(T)[None, :]]
    C = D[:2 * nbins, :win] @ frames
    w = ofe.padded_window(n_fft, win)
    ref = np.fft.rfft(xp[np.arange(n_fft)[:, None] + hop * np.arange(T)[None, :]] * w[:, None], axis=0)
    assert np.max(np.abs(C[:nbins] - ref.real)) <= 1e-6 * np.max(np.abs(ref))
    assert np.max(np.abs(C[nbins:] - ref.imag)) <= 1e-6 * np.max(np.abs(ref))


@pytest.mark.parametrize("n_fft,hop,win", GEOMS)
def test_istft_packed_matrix_is_the_windowed_irfft(n_fft, hop, win):
    nbins = n_fft // 2 + 1
    rtiles, ksteps = -(-win // 32), -(-2 * nbins // 64) * 4
    nb, hi, lo, wsq = _pack_istft(n_fft, hop, win)
    assert nb == ksteps * rtiles * 64 * 16
    E = _unpack(hi, lo, rtiles, ksteps, FE_IE)
    assert not E[win:].any() and not E[:, 2 * nbins:].any(), "padding rows / columns must be exactly zero"
    np.testing.assert_array_equal(wsq, (ofe.hann_periodic(win).astype(np.float32)) ** 2)
    rng = np.random.default_rng(4)
    S = rng.standard_normal((nbins, 9)) + 1j * rng.standard_normal((nbins, 9))
    Y = E[:win, :2 * nbins] @ np.concatenate([S.real, S.imag])
    lpad = (n_fft - win) // 2
    ref = (ofe.padded_window(n_fft, win)[:, None] * np.fft.irfft(S, n=n_fft, axis=0))[lpad:lpad + win]
    assert np.max(np.abs(Y - ref)) <= 1e-6 * np.max(np.abs(ref))


def test_reference_geometry_packed_bytes_unchanged():
    """510/158/400: the same byte counts and the same packed contents as before the general geometries."""
    nb, hi, lo = _pack_stft(510, 158, 400)
    assert nb == 409600
    assert hashlib.sha256(hi.tobytes() + lo.tobytes()).hexdigest() == STFT_REF_SHA256
    nb, hi, lo, wsq = _pack_istft(510, 158, 400)
    assert nb == 425984
    assert hashlib.sha256(hi.tobytes() + lo.tobytes() + wsq.tobytes()).hexdigest() == ISTFT_REF_SHA256


STFT_REF_SHA256 = "7c5afc200dde0fcad9eb66b52d55d68b7e8e72f4e60f20fb2e5a32dc96fc8cca"
ISTFT_REF_SHA256 = "786d08e42dcb003c73056a9322e2ce5fb9e14bfb2e0bdebba39504f0e9922457"


@pytest.mark.parametrize("n_fft,hop,win,rule", REFUSED)
def test_refused_geometries_name_the_rule(n_fft, hop, win, rule):
    h = _lib()
    for fn in (h.sos_stft_matrix_bytes, h.sos_istft_matrix_bytes):
        assert fn(n_fft, hop, win) == -1
        msg = (h.sos_last_error() or b"").decode()
        assert "unsupported geometry" in msg and rule in msg, msg
    buf = np.zeros(16, np.uint16)
    assert h.sos_stft_pack_matrix(n_fft, hop, win, buf.ctypes.data, buf.ctypes.data) != 0
    assert rule in (h.sos_last_error() or b"").decode()
