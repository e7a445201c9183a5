"""Float64 reference of sos_conv2d_fwd (include/sos_hip.h, struct sos_conv_desc) at the kernels' boundary: the buffers as the
descriptor lays them out, the contraction the kernels' channel segments form, the fused epilogue, the storage rounding.
tests/test_conv_reference.py pins it against torch.nn.functional.conv2d in float64; tests/test_gpu_conv_tilings.py compares every
kernel instance and tile geometry with it.

Everything is torch.float64 on the CPU.  A `Case` holds the fields of sos_conv_desc with tensors in place of pointers:
  inp   [B][H][W][in_cs]                 the values the 16-bit input buffer holds
  wgt   [kh*kw][cout_pad][in_nseg*cin]   the values the packed weight buffer holds (engine.pack_weight)
The contraction runs over the channel ranges s < in_nseg: input channels [cin_off + s*in_seg_stride, + cin) against weight columns
[s*cin, (s+1)*cin) -- for the hi|hi|lo activations and hi|lo|hi weights of the bf16x3 mode that is x_hi*w_hi + x_hi*w_lo + x_lo*w_hi
and nothing else: the reference forms the products the kernel forms, not (hi + lo) * (w_hi + w_lo).

EXACT CASES.  reference(case, exact=True) asserts, and raises AssertionError otherwise, that
  * every input and weight value is representable in the storage type,
  * every contraction term is a multiple of 2^-q (q from the values of each segment pair) and the sum of |terms| of every output
    element stays below 2^(24 - q): every partial sum in every order is then an f32 value, so the kernel's f32 accumulators must
    EQUAL the float64 contraction whatever the tiling, the k-step chunking or the order of taps,
  * acc*scale + shift, the activation (ReLU, PReLU; not Sigmoid), the fused input BatchNorm and the accumulation onto the old output
    are f32 values,
  * the fused statistics sum exactly: with the rounded outputs multiples of 2^-s, 384 * max|v| < 2^(24-s) and
    384 * max v^2 < 2^(24-2s) (384: the largest pixel tile a workgroup sums before the tiles are added in double).
An inexact case therefore fails on the CPU and not silently on the GPU."""
from dataclasses import dataclass, field
from typing import Optional

import torch

NONE, RELU, PRELU, SIGMOID = 0, 1, 2, 3          # SOS_ACT_*
ZERO, REFLECT = 0, 1                             # SOS_PAD_*
MAX_TILE = 384                                   # pixel slots of the largest workgroup tile (statistics partial sums)

F64 = torch.float64


def storage_dtype(mode):
    return torch.float16 if mode == "fp16" else torch.bfloat16


def round_storage(v, mode):
    """float64 -> nearest-even value of the 16-bit storage type of `mode` (through f32, as the kernels convert), float64."""
    return v.to(torch.float32).to(storage_dtype(mode)).to(F64)


def split_storage(v, mode):
    """(hi, lo): hi = v rounded to storage, lo = the rest rounded to storage (the hi|hi|lo thirds of the bf16x3 mode)."""
    hi = round_storage(v, mode)
    return hi, round_storage(v.to(torch.float32).to(F64) - hi, mode)


def frac_bits(v, limit=60):
    """Smallest q >= 0 with v * 2^q integral for every element of v (float64 tensor)."""
    v = v.reshape(-1)
    v = v[v != 0]
    for q in range(limit + 1):
        s = v * 2.0 ** q
        if bool((s == s.round()).all()):
            return q
    raise AssertionError("values are not dyadic fractions")


def is_f32(v):
    return bool((v.to(torch.float32).to(F64) == v).all())


def reflect_index(i, n):
    """ReflectionPad2d: -1 -> 1, n -> n - 2 (one reflection)."""
    i = torch.where(i < 0, -i, i)
    return torch.where(i >= n, 2 * (n - 1) - i, i)


@dataclass
class Case:
    inp: torch.Tensor
    wgt: torch.Tensor
    cin: int
    cout: int
    kh: int
    kw: int
    Ho: int
    Wo: int
    cin_off: int = 0
    in_nseg: int = 1
    in_seg_stride: int = 0
    stride: int = 1
    dil_h: int = 1
    dil_w: int = 1
    pad_top: int = 0
    pad_left: int = 0
    pad_mode: int = ZERO
    w_gather: Optional[torch.Tensor] = None      # int64 [Wl] or [B][Wl]: physical column of a logical column
    cout_store: Optional[int] = None             # channels [cout, cout_store) are written as zero
    scale: Optional[torch.Tensor] = None         # [>= cout] each, both or neither
    shift: Optional[torch.Tensor] = None
    act: int = NONE
    slope: float = 0.0
    prev: Optional[torch.Tensor] = None          # accumulate: the value the output held, [B][Ho][Wo][cout_store]
    stats_c: int = 0
    wl_tab: Optional[list] = None                # ragged batch: logical input width / valid output columns per image
    wo_tab: Optional[list] = None
    in_scale: Optional[torch.Tensor] = None      # fused input BatchNorm + ReLU, [cin] each
    in_shift: Optional[torch.Tensor] = None
    extra: dict = field(default_factory=dict)


@dataclass
class Result:
    acc: torch.Tensor        # [B][Ho][Wo][cout] the contraction
    abs_terms: torch.Tensor  # the sum of |w| |x| behind every element of acc
    n_terms: int             # products per output element
    pre: torch.Tensor        # acc*scale + shift
    y: torch.Tensor          # [B][Ho][Wo][cout_store] act(pre), zero filled past cout, before storage rounding
    valid: torch.Tensor      # bool [B][Wo]: the columns the launch writes (ragged batches: wo < wo_tab[b])
    q: int                   # fractional bits of the contraction terms (exact cases)


def contraction(c, exact=True, mode="bf16"):
    """acc, sum of |terms| [B][Ho][Wo][cout_pad'] (cout columns), q."""
    inp = c.inp.to(F64)
    wgt = c.wgt.to(F64)
    B, H, W, _ = inp.shape
    segs = [(c.cin_off + s * c.in_seg_stride, s * c.cin) for s in range(c.in_nseg)]
    if c.in_scale is not None:
        assert c.in_nseg == 1
        a0 = c.cin_off
        z = inp[..., a0:a0 + c.cin] * c.in_scale.to(F64) + c.in_shift.to(F64)
        if exact:
            assert is_f32(z), "fused input BatchNorm: x*scale + shift is not an f32 value"
        inp = inp.clone()
        inp[..., a0:a0 + c.cin] = round_storage(z.clamp_min(0.0), mode)      # as sos_bn_act_apply stores it
    q = 0
    if exact:
        for xo, wo in segs:
            xs, ws = inp[..., xo:xo + c.cin], wgt[:, :c.cout, wo:wo + c.cin]
            assert bool((round_storage(xs, mode) == xs).all()), "input not representable in the storage type"
            assert bool((round_storage(ws, mode) == ws).all()), "weight not representable in the storage type"
            q = max(q, frac_bits(xs) + frac_bits(ws))
    acc = torch.zeros((B, c.Ho, c.Wo, c.cout), dtype=F64)
    tot = torch.zeros_like(acc)
    ho = torch.arange(c.Ho)
    for b in range(B):
        Wl = c.wl_tab[b] if c.wl_tab is not None else (c.w_gather.shape[-1] if c.w_gather is not None else W)
        Wo = c.wo_tab[b] if c.wo_tab is not None else c.Wo
        wo = torch.arange(Wo)
        for a in range(c.kh):
            hi = ho * c.stride - c.pad_top + a * c.dil_h
            if c.pad_mode == REFLECT:
                hi = reflect_index(hi, H)
            hok = (hi >= 0) & (hi < H)
            for t in range(c.kw):
                wi = wo * c.stride - c.pad_left + t * c.dil_w
                if c.pad_mode == REFLECT:
                    wi = reflect_index(wi, Wl)
                wok = (wi >= 0) & (wi < Wl)
                if c.pad_mode == REFLECT:
                    assert bool(hok.all()) and bool(wok.all()), "reflect pad needs a larger input"
                wphys = wi.clamp(0, Wl - 1)
                if c.w_gather is not None:
                    g = c.w_gather if c.w_gather.dim() == 1 else c.w_gather[b]
                    wphys = g[wphys]
                X = inp[b][hi.clamp(0, H - 1)][:, wphys]                                   # [Ho][Wo_b][in_cs]
                X = X * (hok[:, None] & wok[None, :]).to(F64)[:, :, None]
                for xo, wo_ in segs:
                    wt = wgt[a * c.kw + t, :c.cout, wo_:wo_ + c.cin]
                    xs = X[..., xo:xo + c.cin]
                    acc[b, :, :Wo] += xs @ wt.t()
                    tot[b, :, :Wo] += xs.abs() @ wt.abs().t()
    if exact:
        assert float(tot.max()) < 2.0 ** (24 - q), f"sum of |terms| {float(tot.max())} reaches 2^(24 - {q}): not an exact case"
    return acc, tot, q


def reference(c, mode="bf16", exact=True):
    """The float64 result of the launch `c` describes, before storage rounding: Result."""
    acc, tot, q = contraction(c, exact, mode)
    B = acc.shape[0]
    pre = acc
    if c.scale is not None:
        pre = acc * c.scale.to(F64)[:c.cout] + c.shift.to(F64)[:c.cout]
    if c.act == RELU:
        y = pre.clamp_min(0.0)
    elif c.act == PRELU:
        y = torch.where(pre >= 0, pre, c.slope * pre)
    elif c.act == SIGMOID:
        y = torch.sigmoid(pre)
    else:
        y = pre
    y = y + 0.0                                   # (-0 -> +0)
    if exact and c.act != SIGMOID:
        assert is_f32(pre) and is_f32(y), "the epilogue is not exact in f32"
    cs = c.cout if c.cout_store is None else c.cout_store
    full = torch.zeros((B, c.Ho, c.Wo, cs), dtype=F64)
    full[..., :c.cout] = y
    valid = torch.ones((B, c.Wo), dtype=torch.bool)
    if c.wo_tab is not None:
        for b in range(B):
            valid[b, c.wo_tab[b]:] = False
    return Result(acc, tot, c.kh * c.kw * c.in_nseg * c.cin, pre, full, valid, q)


def stored(c, r, mode, out="16", exact=True):
    """What the output buffer holds after the launch, in the channels [out_c_off, out_c_off + cout_store) of the valid columns:
    out = 'f32': the f32 value; else (hi, lo) float64 values of the storage type (lo: the third plane of bf16x3, else None).
    With c.prev the launch accumulates: new = old + the ROUNDED result, split again."""
    if out == "f32":
        assert c.prev is None
        return r.y.to(torch.float32)
    x3 = mode == "bf16x3"
    hi, lo = split_storage(r.y, mode)
    if not x3:
        lo = None
    if c.prev is not None:
        a = hi + (lo if x3 else 0.0) + c.prev.to(F64)
        if exact:
            assert is_f32(a), "accumulation is not exact in f32"
        hi, lo = split_storage(a, mode)
        if not x3:
            lo = None
    return hi, lo


def statistics(c, r, mode, exact=True):
    """[2][stats_c]: sum and sum of squares of the stored (rounded) output over the valid pixels."""
    hi, lo = stored(c, r, mode, exact=exact)
    v = (hi if lo is None else hi + lo)[..., :c.stats_c]
    v = v * r.valid.to(F64)[:, None, :, None]
    if exact:
        s = frac_bits(v)
        assert MAX_TILE * float(v.abs().max()) < 2.0 ** (24 - s), "a tile's sum is not exact in f32"
        assert MAX_TILE * float(v.square().max()) < 2.0 ** (24 - 2 * s), "a tile's sum of squares is not exact in f32"
    return torch.stack([v.sum(dim=(0, 1, 2)), v.square().sum(dim=(0, 1, 2))])


def random_bound(r):
    """|f32 result - reference| <= (n_terms + 2) * 2^-24 * sum |w| |x| for every order of an f32 summation of n_terms exact
    products (+ the two roundings of the epilogue's fma and activation), scale applied by the caller."""
    return (r.n_terms + 2) * 2.0 ** -24 * r.abs_terms


# ------------------------------------------------------------------------------------------------ reproducible inputs
def _hash_int(idx, shape, lo, hi):
    """Integers in [lo, hi], a splitmix-style hash of (idx, element index): reproducible on every platform."""
    import numpy as np
    n = 1
    for s in shape:
        n *= int(s)
    with np.errstate(over="ignore"):
        x = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(idx + 1) * np.uint64(0xBF58476D1CE4E5B9))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    v = (x >> np.uint64(33)) % np.uint64(hi - lo + 1)
    return torch.from_numpy(v.astype(np.int64)).reshape(tuple(shape)) + lo


def exact_input(idx, shape, mode):
    """Activations: integers in [-3, 3]; in bf16x3 mode odd multiples of 2^-9 are added to the nonzero ones so that the value
    needs more than 8 significant bits: hi = the integer, lo = +-2^-9 (below half an ulp of hi, no tie)."""
    a = _hash_int(idx, shape, -3, 3).to(F64)
    if mode == "bf16x3":
        b = _hash_int(idx + 1000, shape, -1, 1).to(F64)
        a = a + torch.where(a != 0, b, torch.zeros_like(b)) * 2.0 ** -9
    return a


def exact_weight(idx, shape, mode):
    """Weights (O, I, kh, kw): integers in [-2, 2] (+ lo = +-2^-9 on the nonzero ones in bf16x3 mode)."""
    a = _hash_int(idx, shape, -2, 2).to(F64)
    if mode == "bf16x3":
        b = _hash_int(idx + 2000, shape, -1, 1).to(F64)
        a = a + torch.where(a != 0, b, torch.zeros_like(b)) * 2.0 ** -9
    return a


def exact_epilogue(cout_pad):
    """scale (powers of two) and shift (multiples of 1/64) [cout_pad]: acc*scale + shift is exact in f32 and needs more than the 11
    significant bits of IEEE half, so the 16-bit outputs see the rounding mode."""
    co = torch.arange(cout_pad)
    return 2.0 ** -(co % 3).to(F64), ((co % 5) - 2).to(F64) / 64.0


def stats_epilogue(cout_pad):
    """Epilogue of the fused-statistics cases: scale 1, integer shifts (with ReLU: the stored outputs stay small integers, or
    halves in bf16x3 mode)."""
    co = torch.arange(cout_pad)
    return torch.ones(cout_pad, dtype=F64), ((co % 3) - 1).to(F64)


def stats_input(idx, shape, mode):
    """Activations of the fused-statistics cases: integers in [-2, 2]; in bf16x3 mode the LAST TWO channels hold 256 +- 1/2
    (hi = 256, lo = +-1/2): stats_weight pairs them with opposite signs, so the large parts cancel and the outputs stay small."""
    a = _hash_int(idx, shape, -2, 2).to(F64)
    if mode == "bf16x3":
        b = _hash_int(idx + 1000, shape[:-1] + (2,), 0, 1).to(F64) - 0.5
        a[..., -2:] = 256.0 + b
    return a


def stats_weight(idx, shape, mode):
    """Weights (O, I, kh, kw) of the fused-statistics cases: one in sixteen is +-1, the rest zero, so that the outputs are small
    integers whose squares sum exactly over a tile; in bf16x3 mode the last two input channels carry +-(1 + 2^-8) at the CENTRE tap
    only (always inside the image) with opposite signs: 256 w_hi and 256 w_lo cancel, x_lo w_hi is +-1/2."""
    O, I, kh, kw = shape
    a = _hash_int(idx, shape, 0, 1).to(F64) * 2.0 - 1.0
    a = a * (_hash_int(idx + 3000, shape, 0, 15) == 0).to(F64)
    if mode == "bf16x3":
        a[:, -2:] = 0.0
        sgn = _hash_int(idx + 4000, (O,), 0, 1).to(F64) * 2.0 - 1.0
        a[:, -2, kh // 2, kw // 2] = sgn * (1.0 + 2.0 ** -8)
        a[:, -1, kh // 2, kw // 2] = -sgn * (1.0 + 2.0 ** -8)
    return a


def pack_weight(w, cin_store, mode, cout_pad=None):
    """engine.pack_weight in float64: (O, I, kh, kw) -> [kh*kw][O_pad][nseg*cin_store]; bf16x3: [w_hi | w_lo | w_hi]."""
    O, I, kh, kw = w.shape
    Op = (O + 31) // 32 * 32 if cout_pad is None else cout_pad
    full = torch.zeros((kh * kw, Op, cin_store), dtype=F64)
    full[:, :O, :I] = w.to(F64).permute(2, 3, 0, 1).reshape(kh * kw, O, I)
    if mode != "bf16x3":
        return round_storage(full, mode)
    hi, lo = split_storage(full, mode)
    return torch.cat([hi, lo, hi], dim=2)


def pack_input(x, cs, mode, cin_off=0, fill=None):
    """(B, H, W, C) float64 -> the input buffer [B][H][W][nseg*cs] with the channels at cin_off of every third: hi | hi | lo in
    bf16x3 mode.  fill: value of the other channels (a reader of the wrong channels gets a wrong sum)."""
    B, H, W, Cc = x.shape
    nseg = 3 if mode == "bf16x3" else 1
    buf = torch.zeros((B, H, W, nseg * cs), dtype=F64) if fill is None else torch.full((B, H, W, nseg * cs), float(fill), dtype=F64)
    hi, lo = split_storage(x, mode)
    buf[..., cin_off:cin_off + Cc] = hi
    if nseg == 3:
        buf[..., cs + cin_off:cs + cin_off + Cc] = hi
        buf[..., 2 * cs + cin_off:2 * cs + cin_off + Cc] = lo
    return buf
