"""Float64 references of the small kernels that move activations and gradients between the big ones, at the kernels' boundary
(tests/test_gpu_glue.py), pinned against torch in tests/test_glue_reference.py:

  csrc/video.hip : sos_time_stack, sos_time_unstack, sos_spatial_mean, sos_spatial_mean_bwd
  csrc/bn.hip    : sos_copy_crop, sos_reflect_fold, sos_reflect_fold_border, sos_pack_grad_f32

Tensors are NHWC rows of the values the buffers actually hold (hi + lo already added in the three-pass mode), on any device;
everything is computed in float64 and nothing here uses the project's code.  The folds are written from the index definition
of reflection (padded cell u mirrors onto row |u - pad|, folded once more at H - 1), not through autograd.

`store` / `split` model one store of a float64 value into a 16-bit buffer of a storage mode: "bf16" and "fp16" round to
nearest even once; "bf16x3" keeps hi = bf16(v) and lo = bf16(v - hi) and holds hi + lo in the thirds hi | hi | lo."""
import torch

NONE, SIGMOID = 0, 3                                       # SOS_ACT_* of include/sos_hip.h
MODES = ("bf16", "fp16", "bf16x3")
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -16}      # relative error of one store (half an ulp)


def _f64(t):
    return torch.as_tensor(t).double()


# ------------------------------------------------------------------------------------------------ storage model
def _dtype(mode):
    return torch.float16 if mode == "fp16" else torch.bfloat16


def _round16(v, mode):
    """float64 -> the 16-bit type in ONE round-to-nearest-even: through f32 rounded to odd (f32 keeps 13 bits more than either
    16-bit type, so the sticky last bit decides every tie the way the exact value would)."""
    v = _f64(v)
    t = v.float()
    over = t.double().abs() > v.abs()                      # rounded away from zero: step one f32 ulp back towards zero
    t = torch.where(over, torch.nextafter(t, torch.zeros_like(t)), t)
    inexact = t.double() != v
    bits = t.view(torch.int32)
    t = torch.where(inexact, bits | 1, bits).view(torch.float32)
    return t.to(_dtype(mode))


def split(v, mode):
    """Bit patterns (int16) of what one store of float64 `v` leaves in a buffer: [..., C] in the 16-bit modes, the thirds
    hi | hi | lo along the last axis ([..., 3 * C]) in the three-pass mode."""
    v = _f64(v)
    hi = _round16(v, mode)
    if mode != "bf16x3":
        return hi.view(torch.int16)
    lo = _round16(v - hi.double(), mode)
    return torch.cat([hi, hi, lo], dim=-1).view(torch.int16)


def store(v, mode):
    """The value (float64) a buffer holds after one store of float64 `v`."""
    v = _f64(v)
    hi = _round16(v, mode).double()
    if mode != "bf16x3":
        return hi
    return hi + _round16(v - hi, mode).double()


def held(bits, mode):
    """The inverse view: the float64 values held by a buffer with the bit patterns of split()."""
    t = bits.view(_dtype(mode)).double()
    if mode != "bf16x3":
        return t
    C = t.shape[-1] // 3
    return t[..., :C] + t[..., 2 * C:]


# ------------------------------------------------------------------------------------------------ video glue
def time_stack(x, kt, out_cs):
    """x [B, T, HW, C] -> [B, T, HW, out_cs]: channel dt * C + c holds frame t + dt - (kt - 1) // 2 of the same clip; zero
    outside the clip and in the channels >= kt * C."""
    x = _f64(x)
    B, T, HW, C = x.shape
    pt = (kt - 1) // 2
    out = torch.zeros(B, T, HW, out_cs, dtype=torch.float64, device=x.device)
    for t in range(T):
        for dt in range(kt):
            ts = t + dt - pt
            if 0 <= ts < T:
                out[:, t, :, dt * C:(dt + 1) * C] = x[:, ts]
    return out


def time_unstack(d, C, kt, in_cs):
    """The transpose of time_stack: d [B, T, HW, st_cs] -> [B, T, HW, in_cs], d_in[t][c] = sum_dt d[t - dt + pt][dt * C + c]
    over the frames of the clip; the stacked channels >= kt * C are ignored, the channels >= C of the result zero."""
    d = _f64(d)
    B, T, HW, _ = d.shape
    pt = (kt - 1) // 2
    out = torch.zeros(B, T, HW, in_cs, dtype=torch.float64, device=d.device)
    for t in range(T):
        for dt in range(kt):
            tf = t - dt + pt
            if 0 <= tf < T:
                out[:, t, :, :C] += d[:, tf, :, dt * C:(dt + 1) * C]
    return out


def time_unstack_abs(d, C, kt, in_cs):
    """Sum of |terms| of time_unstack (for the tolerance of the sum)."""
    return time_unstack(_f64(d).abs(), C, kt, in_cs)


def spatial_mean(x):
    """x [N, HW, C] -> [N, C], the mean over the pixels."""
    x = _f64(x)
    return x.sum(1) / x.shape[1]


def spatial_mean_bwd(dfeat, HW, cs):
    """dfeat [N, C] -> [N, HW, cs]: every pixel gets dfeat / HW, the channels >= C zero."""
    dfeat = _f64(dfeat)
    N, C = dfeat.shape
    out = torch.zeros(N, HW, cs, dtype=torch.float64, device=dfeat.device)
    out[..., :C] = (dfeat / HW)[:, None, :]
    return out


# ------------------------------------------------------------------------------------------------ crop and folds
def copy_crop(src, Hd, Wd):
    """src [B, Hs, Ws, C] -> [B, Hd, Wd, C]: the overlap copied, the rest zero."""
    src = _f64(src)
    B, Hs, Ws, C = src.shape
    out = torch.zeros(B, Hd, Wd, C, dtype=torch.float64, device=src.device)
    h, w = min(Hs, Hd), min(Ws, Wd)
    out[:, :h, :w] = src[:, :h, :w]
    return out


def _mirror(u, pad, n):
    """Interior index that cell u of a reflect-padded axis (n interior cells, pad <= n - 1) reads."""
    i = abs(u - pad)
    return 2 * (n - 1) - i if i > n - 1 else i


def _fold(padded, H, W, pad, border_only):
    """(sum, sum of |terms|, number of terms) [B, H, W, C] / [H, W] of the padded cells that mirror onto every interior cell."""
    padded = _f64(padded)
    B, Hp, Wp, C = padded.shape
    assert Hp == H + 2 * pad and Wp == W + 2 * pad and 0 <= pad < min(H, W)
    dev = padded.device
    s = torch.zeros(B, H, W, C, dtype=torch.float64, device=dev)
    a = torch.zeros_like(s)
    n = torch.zeros(H, W, dtype=torch.float64, device=dev)
    wmap = torch.tensor([_mirror(v, pad, W) for v in range(Wp)], device=dev)
    for u in range(Hp):                                    # one padded row at a time, its cells scattered onto the columns
        h = _mirror(u, pad, H)
        row = padded[:, u].clone()
        one = torch.ones(Wp, dtype=torch.float64, device=dev)
        if border_only and pad <= u < pad + H:             # the cells (h + pad, w + pad) are the interior itself
            row[:, pad:pad + W] = 0.0
            one[pad:pad + W] = 0.0
        s[:, h].index_add_(1, wmap, row)
        a[:, h].index_add_(1, wmap, row.abs())
        n[h].index_add_(0, wmap, one)
    return s, a, n.long().cpu()


def reflect_fold(padded, H, W, pad, out=None, accumulate=False, terms=False):
    """Backward of ReflectionPad2d(pad): padded [B, H + 2 pad, W + 2 pad, C] folded onto [B, H, W, C], added to `out` when
    `accumulate`.  terms=True: also the sum of |terms| and the largest number of terms of a cell."""
    s, a, n = _fold(padded, H, W, pad, False)
    k = int(n.max())
    if accumulate:
        s, a, k = s + _f64(out).to(s.device), a + _f64(out).to(s.device).abs(), k + 1
    return (s, a, k) if terms else s


def reflect_fold_border(padded, H, W, pad, out, terms=False):
    """out + the BORDER cells of `padded` folded onto the interior cells they mirror (the cell (h + pad, w + pad) itself is not
    added: the convolution wrote it).  Cells without a mirrored border cell keep `out`."""
    s, a, n = _fold(padded, H, W, pad, True)
    o = _f64(out).to(s.device)
    return (s + o, a + o.abs(), int(n.max()) + 1) if terms else s + o


def fold_touched(H, W, pad):
    """bool [H, W]: the interior cells that have a mirrored border cell (the ones sos_reflect_fold_border may write)."""
    t = torch.zeros(H, W, dtype=torch.bool)
    for u in range(H + 2 * pad):
        for v in range(W + 2 * pad):
            h, w = _mirror(u, pad, H), _mirror(v, pad, W)
            if u != h + pad or v != w + pad:
                t[h, w] = True
    return t


# ------------------------------------------------------------------------------------------------ f32 gradient pack
def pack_grad(g, y, act, outer, inner, C, so, st, sc, mul=1.0):
    """Rows [outer * inner, C] of the FLOAT32 products the kernel stores: element (o, t, c) is g[o so + t st + c sc] * mul
    (* y (1 - y) at the same address for SIGMOID), multiplied in f32 in that order.  `g` / `y`: flat f32 tensors."""
    g = torch.as_tensor(g).float().reshape(-1)
    o = torch.arange(outer, device=g.device)[:, None, None]
    t = torch.arange(inner, device=g.device)[None, :, None]
    c = torch.arange(C, device=g.device)[None, None, :]
    idx = (o * so + t * st + c * sc).reshape(outer * inner, C)
    v = g[idx] * torch.tensor(mul, dtype=torch.float32, device=g.device)
    if act == SIGMOID:
        yy = torch.as_tensor(y).float().reshape(-1)[idx]
        v = v * (yy * (1.0 - yy))
    else:
        assert act == NONE, act
    return v


# ------------------------------------------------------------------------------------------------ tolerance of a stored sum
def sum_tol(want, abs_terms, n, mode, divisor=1.0):
    """|got - want| allowed for a sum of n exactly representable terms accumulated in f32, divided by `divisor` and stored
    once: u |want| + 4 n 2^-24 sum|x_i| / divisor (+ the subnormal spacing 2^-24 in IEEE half)."""
    tol = UNIT[mode] * _f64(want).abs() + 4.0 * n * 2.0 ** -24 * _f64(abs_terms) / divisor
    return tol + 2.0 ** -24 if mode == "fp16" else tol


def f32_term(abs_terms, n, divisor=1.0):
    """The f32 accumulation part of sum_tol alone."""
    return 4.0 * n * 2.0 ** -24 * _f64(abs_terms) / divisor
