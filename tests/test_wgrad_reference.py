"""tests/wgrad_reference.py against torch float64 autograd (CPU): conv2d with stride / dilation / zero and reflection padding,
padding independent of the kernel size, channel strides and offsets with NaN neighbours, the ConvTranspose2d role swap, the temporal
taps (conv3d), scale / accumulate, the three bf16x3 passes, the term count and the exactness condition."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_reference as R

from util import hashed

TOL = 1e-12          # float64 sums of a few thousand terms of magnitude <= 1, two summation orders


def _nhwc(t, cs, off):
    """NCHW float64 tensor -> NHWC numpy array of cs channels, the tensor's at [off, off + C), NaN elsewhere."""
    B, Cc, H, W = t.shape
    a = np.full((B, H, W, cs), np.nan)
    a[..., off:off + Cc] = t.permute(0, 2, 3, 1).numpy()
    return a


def _rand(idx, shape):
    return torch.from_numpy(hashed(idx, shape).astype(np.float64))


CONV_CASES = [
    # name, M, N, k, stride, dil, pad, reflect, H, W
    ("3x3 same", 5, 7, (3, 3), 1, (1, 1), (1, 1), False, 9, 11),
    ("5x5 dil(2,3)", 4, 6, (5, 5), 1, (2, 3), (4, 6), False, 13, 17),
    ("5x5 s2 reflect", 6, 3, (5, 5), 2, (1, 1), (2, 2), True, 11, 14),
    ("3x3 s2 zero", 3, 5, (3, 3), 2, (1, 1), (1, 1), False, 10, 13),
    ("3x3 reflect", 2, 9, (3, 3), 1, (1, 1), (1, 1), True, 7, 8),
    ("7x1", 5, 4, (7, 1), 1, (1, 1), (3, 0), False, 12, 9),
    ("5x1 dil2 reflect", 4, 3, (5, 1), 1, (2, 1), (4, 0), True, 9, 8),
    ("1x1", 7, 9, (1, 1), 1, (1, 1), (0, 0), False, 5, 6),
    ("5x5 dilation beyond the image", 3, 4, (5, 5), 1, (8, 9), (16, 18), False, 7, 10),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_reference_equals_conv2d_autograd(case):
    _, M, N, k, stride, dil, pad, reflect, H, W = case
    B = 2
    x = _rand(11, (B, N, H, W))
    xp = F.pad(x, (pad[1], pad[1], pad[0], pad[0]), mode="reflect") if reflect else x
    w = torch.zeros(M, N, *k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xp, w, None, stride, (0, 0) if reflect else pad, dil)
    g = _rand(12, tuple(y.shape))
    y.backward(g)
    ga, xa = _nhwc(g, M + 24, 8), _nhwc(x, N + 16, 16)
    dw, sabs, nterms = R.reference(ga, xa, g_off=8, M=M, x_off=16, N=N, kh=k[0], kw=k[1], stride=stride, dil=dil, pad=pad,
                                   pad_mode=R.REFLECT if reflect else R.ZERO)
    assert np.max(np.abs(dw - w.grad.numpy())) < TOL * max(1.0, float(sabs.max()))
    assert (np.abs(dw) <= sabs + 1e-15).all() and nterms.max() <= B * y.shape[2] * y.shape[3]
    # scale and accumulate
    dw0 = hashed(13, dw.shape)
    dw2, _, _ = R.reference(ga, xa, g_off=8, M=M, x_off=16, N=N, kh=k[0], kw=k[1], stride=stride, dil=dil, pad=pad,
                            pad_mode=R.REFLECT if reflect else R.ZERO, scale=0.25, dw0=dw0)
    assert np.max(np.abs(dw2 - (dw0 + 0.25 * w.grad.numpy()))) < TOL * max(1.0, float(sabs.max()))


def test_padding_is_independent_of_the_kernel_size():
    """pad_top / pad_left are the descriptor's own: an asymmetric padding (3 rows above, 1 column left of a 3x3 kernel)."""
    B, M, N, H, W = 2, 3, 4, 8, 9
    x = _rand(21, (B, N, H, W))
    xp = F.pad(x, (1, 4, 3, 2))                      # left 1, right 4, top 3, bottom 2
    w = torch.zeros(M, N, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xp, w)
    g = _rand(22, tuple(y.shape))
    y.backward(g)
    dw, _, _ = R.reference(_nhwc(g, M, 0), _nhwc(x, N, 0), g_off=0, M=M, x_off=0, N=N, kh=3, kw=3, pad=(3, 1))
    assert y.shape[2] == H + 3 and np.max(np.abs(dw - w.grad.numpy())) < 1e-11


def test_conv_transpose_role_swap():
    """ConvTranspose2d(k3, s2, p1, output_padding 1): G = the layer input (Hg x Wg), X = the output gradient (2 Hg x 2 Wg),
    stride 2, pad 1; the result is already in the (Cin, Cout, kh, kw) layout."""
    B, Cin, Cout, H, W = 2, 5, 3, 6, 7
    x = _rand(31, (B, Cin, H, W))
    w = torch.zeros(Cin, Cout, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, None, 2, 1, 1)
    assert tuple(y.shape[2:]) == (2 * H, 2 * W)
    g = _rand(32, tuple(y.shape))
    y.backward(g)
    dw, _, _ = R.reference(_nhwc(x, Cin + 8, 8), _nhwc(g, Cout + 8, 0), g_off=8, M=Cin, x_off=0, N=Cout, kh=3, kw=3, stride=2,
                           pad=(1, 1))
    assert np.max(np.abs(dw - w.grad.numpy())) < 1e-11


@pytest.mark.parametrize("kt", [3, 5])
def test_temporal_taps_equal_conv3d(kt):
    B, T, I, O, H, W = 2, 4, 6, 3, 5, 6
    x = _rand(41, (B, I, T, H, W))
    w = torch.zeros(O, I, kt, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, w, None, 1, ((kt - 1) // 2, 1, 1))
    g = _rand(42, tuple(y.shape))
    y.backward(g)
    frames = lambda t: t.permute(0, 2, 1, 3, 4).reshape(B * T, t.shape[1], H, W)
    dw, _, _ = R.reference(_nhwc(frames(g), O, 0), _nhwc(frames(x), I + 8, 8), g_off=0, M=O, x_off=8, N=kt * I, kh=3, kw=3, pad=(1, 1),
                           temporal=(T, kt, (kt - 1) // 2, I))
    want = w.grad.permute(0, 2, 1, 3, 4).reshape(O, kt * I, 3, 3).numpy()
    assert np.max(np.abs(dw - want)) < 1e-11


def test_x3_passes_are_hi_hi_plus_hi_lo_plus_lo_hi():
    """The three passes over hi|hi|lo thirds: (g_hi + g_lo)(x_hi + x_lo) WITHOUT the lo*lo term, as engine.wgrad launches them."""
    B, M, N, H, W, cs_g, cs_x = 2, 3, 4, 6, 7, 8, 8
    parts = {n: _rand(50 + i, (B, c, H, W)) for i, (n, c) in enumerate((("gh", M), ("gl", M), ("xh", N), ("xl", N)))}
    w = torch.zeros(M, N, 3, 3, dtype=torch.float64, requires_grad=True)
    y = (F.conv2d(parts["xh"], w, None, 1, 1), F.conv2d(parts["xl"], w, None, 1, 1))
    (y[0] * (parts["gh"] + parts["gl"])).sum().backward()
    (y[1] * parts["gh"]).sum().backward()
    g = np.concatenate([_nhwc(parts["gh"], cs_g, 0), _nhwc(parts["gh"], cs_g, 0), _nhwc(parts["gl"], cs_g, 0)], axis=3)
    x = np.concatenate([_nhwc(parts["xh"], cs_x, 0), _nhwc(parts["xh"], cs_x, 0), _nhwc(parts["xl"], cs_x, 0)], axis=3)
    dw, sabs, nterms = R.reference_x3(g, x, cs_g, cs_x, g_off=0, M=M, x_off=0, N=N, kh=3, kw=3, pad=(1, 1))
    assert np.max(np.abs(dw - w.grad.numpy())) < 1e-11
    one, s1, n1 = R.reference(g, x, g_off=0, M=M, x_off=0, N=N, kh=3, kw=3, pad=(1, 1))
    assert (sabs >= s1).all() and (nterms <= 3 * B * H * W).all() and (nterms >= n1).all()


def test_term_count_and_exactness_condition():
    """nterms counts the non-zero products only; assert_exact accepts the test grid up to 16 384 pixels of full-magnitude products
    and refuses what could round."""
    g = np.zeros((1, 2, 3, 8))
    x = np.zeros((1, 2, 3, 8))
    g[0, 0, 0, 0], g[0, 1, 2, 0] = 0.5, -0.25
    x[0, 0, 0, 1], x[0, 1, 2, 1], x[0, 1, 1, 1] = 1.0, 0.75, 1.0
    dw, sabs, nterms = R.reference(g, x, g_off=0, M=1, x_off=1, N=1, kh=1, kw=1)
    assert dw[0, 0, 0, 0] == 0.5 - 0.1875 and sabs[0, 0, 0, 0] == 0.5 + 0.1875 and nterms[0, 0, 0, 0] == 2
    gv, xl = R.grid_values(1, (4000,)), R.grid_values(2, (4000,), step=2.0 ** -8)
    assert set(np.unique(gv * 4)) == set(range(-4, 5)) and np.abs(xl).max() == 2.0 ** -6
    assert R.assert_exact(gv, xl, np.array([16383.0])) == 10
    with pytest.raises(AssertionError):
        R.assert_exact(gv, xl, np.array([16384.0]))
    with pytest.raises(AssertionError):
        R.assert_exact(gv, xl, np.array([10.0]), scale=0.3)
    with pytest.raises(AssertionError):
        R.assert_exact(gv, gv, np.array([10.0]), scale=0.5, dw0=np.array([1.0 / 64]))      # not a multiple of 2^-4 / 2
    R.assert_exact(gv, gv, np.array([10.0]), scale=0.5, dw0=np.array([3.0 / 32]))
