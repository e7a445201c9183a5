"""STFT / ISTFT kernels (csrc/stft_mfma.hip) at librosa geometries other than the reference's 510/158/400: against the
float64 oracle, round trip, ragged batches with NaN sentinels, determinism, full size, the numpy mirrors, refusals."""
import numpy as np
import pytest
import torch

from oracle import frontend as ofe

pytestmark = pytest.mark.gpu

# (n_fft, hop, win)
GEOMS = [(512, 128, 512),      # BASELINE's 16 kHz STFT(512/128)
         (400, 160, 400),      # n_fft + 2 not a multiple of 32
         (510, 128, 400),      # the networks' 256 bins at a 16 kHz hop, overlap 4
         (256, 64, 256),       # overlap 4
         (1024, 256, 1024),
         (2048, 512, 2048),    # 65 STFT and 64 ISTFT row tiles
         (2048, 128, 2048),    # overlap 16, the limit
         (512, 128, 301),      # odd window, not a multiple of 16
         (882, 441, 882),      # odd hop
         (510, 157, 400),      # odd hop at the reference bins
         (256, 256, 256),      # no overlap
         (256, 200, 160),      # hop > win: gaps
         (16, 4, 16)]          # smallest
# the window-sum-square has zeros (w[0] = 0 without overlap) or gaps: the round trip does not return x there
NO_NOLA = ((256, 256, 256), (256, 200, 160))
REFUSED = [(511, 128, 511), (512, 128, 513), (512, 128, 15), (512, 0, 512), (512, 513, 512), (2048, 127, 2048),
           (4096, 1024, 4096)]

# max |kernel - oracle| / max |oracle| per clip.  Observed on MI355X, worst over the geometries: STFT 1.2e-6 (2048/128/2048);
# ISTFT 1.2e-6 (2048/512/2048), 6.0e-6 without overlap (256/256/256: a random spectrogram divided by wss down to w[1]^2)
STFT_TOL = 1e-5
ISTFT_TOL = 1e-5
# max |istft(stft(x)) - x| / max |x| where NOLA holds.  Observed: 8.8e-7 (2048/512/2048)
ROUNDTRIP_TOL = 2e-5


def _n_samples(hop):
    return max(16000, 150 * hop)                  # at least two frame tiles of 64 at every hop


def _waves(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N, generator=g, dtype=torch.float64) * 0.1).float()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _oracle_stft(x, g):
    return ofe.real_imag_expand(ofe.stft_complex(x, *g)).transpose(2, 0, 1)           # (2, F, T)


def _oracle_istft(S, g):
    return ofe.istft_complex(S[0].astype(np.float64) + 1j * S[1].astype(np.float64), g[1], g[2])


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: "%d-%d-%d" % g)
def test_stft_istft_against_oracle(g):
    from sos_amd import transform as T
    n_fft, hop, win = g
    N, B = _n_samples(hop), 3
    w = _waves(B, N, 11)
    S = T.stft_batch(w.cuda(), n_fft, hop, win)
    assert S.shape == (B, 2, n_fft // 2 + 1, 1 + N // hop)
    Sc = S.cpu().numpy()
    for b in range(B):
        e = _rel(Sc[b], _oracle_stft(w[b].numpy(), g))
        assert e <= STFT_TOL, (g, b, e)
    # ISTFT of a seeded random spectrogram and of the STFT output
    Sr = _waves(B * 2 * (n_fft // 2 + 1), S.shape[-1], 12).reshape(S.shape)
    wss = ofe.window_sumsquare(S.shape[-1], n_fft, hop, win)[n_fft // 2:-(n_fft // 2)]
    for spec in (Sr, torch.from_numpy(Sc)):
        y = T.istft_batch(spec.cuda(), hop, win).cpu().numpy()
        assert y.shape == (B, hop * (S.shape[-1] - 1))
        for b in range(B):
            yo = _oracle_istft(spec[b].numpy(), g)
            if g in NO_NOLA and spec is not Sr:
                # x = y / wss where wss is as small as w[1]^2 = 6e-8: the division magnifies f32 rounding of y there, in
                # the oracle too.  Compare the overlap-add before the division; samples in gaps are 0 in both.
                e = _rel(y[b] * wss, yo * wss)
                gap = wss <= np.finfo(np.float32).tiny
                assert np.array_equal(y[b][gap], yo[gap]), (g, b)
            else:
                e = _rel(y[b], yo)
            assert e <= ISTFT_TOL, (g, b, e)
    if g not in NO_NOLA:
        for b in range(B):
            x = w[b, :y.shape[1]].numpy()
            e = float(np.max(np.abs(y[b] - x)) / np.max(np.abs(x)))
            assert e <= ROUNDTRIP_TOL, (g, b, e)


def _stft_into(w, g, clip_samples, out):
    from sos_amd import _lib as L, transform as T
    mhi, mlo = T._front_tables(w.device, *g)
    B, N = w.shape
    L.check(L.lib().sos_stft_f32(L.ptr(w), B, N, N, L.ptr(mhi), L.ptr(mlo), g[0], g[1], g[2], L.ptr(out), out.shape[-1],
                                 L.ptr(clip_samples), L.stream_ptr()), "sos_stft_f32")
    return out


def _istft_into(spec, g, clip_frames, out):
    from sos_amd import _lib as L, transform as T
    mhi, mlo, wsq = T._front_tables(spec.device, *g, inverse=True)
    B, _, F, Tn = spec.shape
    L.check(L.lib().sos_istft_f32(L.ptr(spec), B, Tn, L.ptr(mhi), L.ptr(mlo), L.ptr(wsq), g[0], g[1], g[2], L.ptr(out),
                                  out.shape[-1], L.ptr(clip_frames), L.stream_ptr()), "sos_istft_f32")
    return out


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: "%d-%d-%d" % g)
def test_ragged_batches_match_single_clips_and_keep_sentinels(g):
    from sos_amd import transform as T
    n_fft, hop, win = g
    N = _n_samples(hop)
    lens = [N, N - 3 * hop - 5, 20 * hop + 7 if 20 * hop + 7 > n_fft // 2 else n_fft // 2 + 1, N // 2 + 1]
    B = len(lens)
    w = _waves(B, N, 21).cuda()
    Tn = 1 + N // hop
    cs = torch.tensor(lens, dtype=torch.int32, device="cuda")
    S = _stft_into(w, g, cs, torch.full((B, 2, n_fft // 2 + 1, Tn), float("nan"), device="cuda"))
    tf = [1 + n // hop for n in lens]
    for b, n in enumerate(lens):
        one = T.stft_batch(w[b:b + 1, :n].contiguous(), n_fft, hop, win)[0]
        assert torch.equal(S[b, :, :, :tf[b]], one), (g, b)
        assert torch.isnan(S[b, :, :, tf[b]:]).all(), (g, b)
    spec = torch.nan_to_num(S, nan=0.0)
    cf = torch.tensor(tf, dtype=torch.int32, device="cuda")
    y = _istft_into(spec, g, cf, torch.full((B, hop * (Tn - 1)), float("nan"), device="cuda"))
    for b, t in enumerate(tf):
        one = T.istft_batch(spec[b:b + 1, :, :, :t].contiguous(), hop, win)[0]
        assert torch.equal(y[b, :hop * (t - 1)], one), (g, b)
        assert torch.isnan(y[b, hop * (t - 1):]).all(), (g, b)


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: "%d-%d-%d" % g)
def test_determinism_and_batch_independence(g):
    from sos_amd import transform as T
    n_fft, hop, win = g
    N = min(_n_samples(hop), 20000)
    w = _waves(64, N, 31).cuda()
    S1, S2 = T.stft_batch(w, n_fft, hop, win), T.stft_batch(w, n_fft, hop, win)
    assert torch.equal(S1, S2)
    y1, y2 = T.istft_batch(S1, hop, win), T.istft_batch(S1, hop, win)
    assert torch.equal(y1, y2)
    for b in (0, 29, 63):
        assert torch.equal(T.stft_batch(w[b:b + 1].contiguous(), n_fft, hop, win)[0], S1[b])
        assert torch.equal(T.istft_batch(S1[b:b + 1].contiguous(), hop, win)[0], y1[b])


@pytest.mark.parametrize("g", [(512, 128, 512), (1024, 256, 1024)], ids=lambda g: "%d-%d-%d" % g)
def test_full_size_batch(g):
    from sos_amd import transform as T
    n_fft, hop, win = g
    w = _waves(64, 32000, 41)
    S = T.stft_batch(w.cuda(), n_fft, hop, win)
    assert S.shape == (64, 2, n_fft // 2 + 1, 1 + 32000 // hop)
    y = T.istft_batch(S, hop, win).cpu().numpy()
    Sc = S.cpu().numpy()
    for b in (0, 17, 63):
        assert _rel(Sc[b], _oracle_stft(w[b].numpy(), g)) <= STFT_TOL, b
        assert _rel(y[b], _oracle_istft(Sc[b], g)) <= ISTFT_TOL, b


@pytest.mark.parametrize("g", [(512, 128, 512), (882, 441, 882)], ids=lambda g: "%d-%d-%d" % g)
def test_numpy_mirrors(g):
    from sos_amd import transform as T
    n_fft, hop, win = g
    x = _waves(1, 32000, 51)[0].numpy()
    F = T.fast_stft(x, n_fft=n_fft, hop_length=hop, win_length=win)
    ref = ofe.fast_stft(x, n_fft, hop, win)
    assert F.shape == ref.shape and _rel(F, ref) <= STFT_TOL
    Fp = T.fast_stft(x, power=True, n_fft=n_fft, hop_length=hop, win_length=win)
    assert _rel(Fp, ofe.fast_stft(ofe.power_law(x.astype(np.float32), 0.3), n_fft, hop, win)) <= STFT_TOL
    y = T.fast_istft(ref, hop_length=hop, win_length=win)
    yref = ofe.fast_istft(ref, hop, win)
    assert y.dtype == np.float32 and y.shape == yref.shape and _rel(y, yref) <= ISTFT_TOL
    yp = T.fast_istft(ref, power=True, hop_length=hop, win_length=win)
    assert yp.dtype == np.float64 and _rel(yp, ofe.power_law(yref, 1.0 / 0.3)) <= 1e-4


@pytest.mark.parametrize("g", REFUSED, ids=lambda g: "%d-%d-%d" % g)
def test_refused_geometries_raise_before_any_launch(g, monkeypatch):
    from sos_amd import transform as T
    n_fft, hop, win = g

    def launched(*a, **k):
        raise AssertionError("launched for a refused geometry")
    monkeypatch.setattr(T, "_front_tables", launched)
    monkeypatch.setattr(T, "power_law_batch", launched)
    w = torch.zeros(1, 4096, device="cuda")
    with pytest.raises(ValueError, match="unsupported geometry"):
        T.stft_batch(w, n_fft, hop, win)
    with pytest.raises(ValueError, match="unsupported geometry"):
        T.fast_stft(np.zeros(4096, np.float32), power=True, n_fft=n_fft, hop_length=hop, win_length=win)
    spec = torch.zeros(1, 2, n_fft // 2 + 1, 4, device="cuda")       # istft_batch infers n_fft = 2*(F-1): always even
    if n_fft % 2 == 0:
        with pytest.raises(ValueError, match="unsupported geometry"):
            T.istft_batch(spec, hop, win)
        with pytest.raises(ValueError, match="unsupported geometry"):
            T.fast_istft(np.zeros((n_fft // 2 + 1, 4, 2)), power=True, hop_length=hop, win_length=win)
