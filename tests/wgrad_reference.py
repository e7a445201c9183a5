"""Float64 reference of sos_conv2d_wgrad (include/sos_hip.h, struct sos_wgrad_desc) at the kernels' boundary:

    dw[m][n][a][b] (+)= scale * sum over pixels p of  G[p][g_off + m] * X[p * stride + (a, b) * dil - pad][x_off + n]

on the NHWC arrays as the descriptor lays them out (channel strides g_cs / x_cs, first owned channels g_off / x_off; no channel
outside [off, off + M) is ever read, so the caller may fill the neighbours with NaN).  Plain numpy, one gather and one matrix product
per tap.  tests/test_wgrad_reference.py pins it against torch float64 autograd; tests/test_gpu_wgrad_plans.py compares every route,
kernel instance and plan of csrc/wgrad.hip with it.

Besides dw it returns, per element, sabs = sum |G| |X| over the terms and nterms = the number of non-zero terms: the bound of the
rounding test ((nterms + ...) 2^-24 sabs) and the exactness condition below are stated in them.

EXACT CASES.  assert_exact() raises AssertionError unless every product is a multiple of one power of two (the quantum) and sabs /
quantum < 2^24 for every element: then every partial sum of the products, in every order and through every split, is an f32 value
and the kernels' f32 accumulators must EQUAL the float64 sum bit for bit, whatever route, plan or pixel split ran.  scale must be a
power of two and an accumulated-onto dw a multiple of scale * quantum with |dw| + |scale| sabs below 2^24 quanta."""
import numpy as np

ZERO, REFLECT = 0, 1                             # SOS_PAD_*
X3_PASSES = ((0, 0), (0, 2), (2, 0))             # engine.wgrad: (third of G, third of X) = hi*hi, hi*lo, lo*hi, in this order


def reflect_index(i, n):
    """reflect_index() of csrc/sos_common.h: -1 -> 1, n -> n - 2, then clamped into the image."""
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def _tap_index(n_out, n_in, stride, shift, reflect):
    """Source coordinate of every output coordinate for one tap, and which of them lie inside the image."""
    i = np.arange(n_out) * stride + shift
    if reflect:
        return reflect_index(i, n_in), np.ones(n_out, bool)
    ok = (i >= 0) & (i < n_in)
    return np.where(ok, i, 0), ok


def reference(g, x, *, g_off, M, x_off, N, kh, kw, stride=1, dil=(1, 1), pad=(0, 0), pad_mode=ZERO, temporal=None, scale=1.0,
              dw0=None):
    """(dw, sabs, nterms), each float64 [M][N][kh][kw].  g: [B][Hg][Wg][g_cs], x: [B][Hx][Wx][x_cs] (anything numpy converts).
    temporal = (frames per clip, taps, t_pad, channels per frame): column n = dt * t_cin + c pairs image b of G with channel c of
    frame b + dt - t_pad of X, zeros outside the clip.  dw0: the gradient accumulated onto (accumulate = 1), else accumulate = 0."""
    g = np.asarray(g, np.float64)
    x = np.asarray(x, np.float64)
    B, Hg, Wg, _ = g.shape
    Bx, Hx, Wx, _ = x.shape
    assert B == Bx
    G = g[..., g_off:g_off + M].reshape(-1, M)
    assert G.shape[1] == M and not np.isnan(G).any(), "owned channels of G"
    if temporal is None:
        cols = [(0, x[..., x_off:x_off + N])]
        ncol = N
    else:
        T, kt, tpad, tcin = temporal
        assert N == kt * tcin and B % T == 0
        xc = x[..., x_off:x_off + tcin]
        cols = []
        for dt in range(kt):
            fr = np.arange(B) % T + dt - tpad
            ok = (fr >= 0) & (fr < T)
            src = np.where(ok, np.arange(B) + dt - tpad, 0)
            cols.append((dt * tcin, xc[src] * ok[:, None, None, None]))
        ncol = tcin
    for _, xs in cols:
        assert xs.shape[-1] == ncol and not np.isnan(xs).any(), "owned channels of X"
    dw = np.zeros((M, N, kh, kw))
    sabs = np.zeros((M, N, kh, kw))
    nterms = np.zeros((M, N, kh, kw))
    Ga, Gn = np.abs(G), (G != 0).astype(np.float64)
    reflect = pad_mode == REFLECT
    for a in range(kh):
        hi, hok = _tap_index(Hg, Hx, stride, a * dil[0] - pad[0], reflect)
        for b in range(kw):
            wi, wok = _tap_index(Wg, Wx, stride, b * dil[1] - pad[1], reflect)
            ok = (hok[:, None] & wok[None, :])[None, :, :, None]
            for n0, xs in cols:
                X = (xs[:, hi][:, :, wi] * ok).reshape(-1, ncol)
                dw[:, n0:n0 + ncol, a, b] = G.T @ X
                sabs[:, n0:n0 + ncol, a, b] = Ga.T @ np.abs(X)
                nterms[:, n0:n0 + ncol, a, b] = Gn.T @ (X != 0).astype(np.float64)
    dw = dw * scale
    if dw0 is not None:
        dw = np.asarray(dw0, np.float64) + dw
    return dw, sabs, nterms


def reference_x3(g, x, g_third, x_third, *, g_off, x_off, scale=1.0, dw0=None, **kw):
    """The bf16x3 mode as engine.wgrad runs it: three accumulating launches over the hi|hi|lo thirds (channel capacity g_third /
    x_third each) -- hi*hi, hi*lo, lo*hi and nothing else.  Returns the sums of the three passes' (dw, sabs, nterms)."""
    dw = None if dw0 is None else np.asarray(dw0, np.float64)
    sabs = nterms = 0.0
    for gt, xt in X3_PASSES:
        dw, s, n = reference(g, x, g_off=g_off + gt * g_third, x_off=x_off + xt * x_third, scale=scale, dw0=dw, **kw)
        sabs, nterms = sabs + s, nterms + n
    return dw, sabs, nterms


def frac_bits(v, limit=60):
    """Smallest q >= 0 with v * 2^q integral for every element."""
    v = np.asarray(v, np.float64).reshape(-1)
    v = v[v != 0]
    for q in range(limit + 1):
        s = v * 2.0 ** q
        if (s == np.round(s)).all():
            return q
    raise AssertionError("values are not dyadic fractions")


def is_pow2(v):
    m, _ = np.frexp(abs(float(v)))
    return m == 0.5


def assert_exact(g_owned, x_owned, sabs, scale=1.0, dw0=None):
    """The exactness condition of the module docstring.  g_owned / x_owned: every value a launch multiplies -- for bf16x3 a list of
    (g values, x values) per pass.  Returns the fractional bits q of the quantum 2^-q."""
    pairs = g_owned if isinstance(g_owned, list) else [(g_owned, x_owned)]
    q = max(frac_bits(gv) + frac_bits(xv) for gv, xv in pairs)
    worst = float(np.max(sabs)) * 2.0 ** q
    assert worst < 2.0 ** 24, f"sum |g||x| reaches {worst:.0f} quanta of 2^-{q}: partial sums may round"
    assert is_pow2(scale), "scale must be a power of two"
    if dw0 is not None:
        unit = abs(scale) * 2.0 ** -q
        d = np.asarray(dw0, np.float64)
        assert (d / unit == np.round(d / unit)).all(), "dw0 is not a multiple of scale * quantum"
        assert float(np.max(np.abs(d) + abs(scale) * sabs)) / unit < 2.0 ** 24, "accumulating onto dw0 may round"
    return q


def grid_values(idx, shape, step=0.25, kmax=4):
    """Deterministic values k * step, |k| <= kmax, from a multiplicative hash of the flat index (no RNG state)."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    h = (i + np.uint64(idx) * np.uint64(0x9E3779B1)) * np.uint64(0x85EBCA6B)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    k = (h % np.uint64(2 * kmax + 1)).astype(np.int64) - kmax
    return (k.astype(np.float64) * step).reshape(shape)
