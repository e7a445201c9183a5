"""The BatchNorm + activation kernels of csrc/bn.hip against the float64 reference of tests/bn_reference.py, on every launch path:

  forward : sos_bn_stats (1 .. 2048 workgroups, the cap, many strides per lane and the BN_U tail) + sos_bn_finalize
            (bn_finalize_kernel<256> / <1024>, the 4-way loop and its tail; count = 1 is train_ops.colsum), the statistics fused
            into the conv epilogue (the training path of the full-resolution encoder blocks: below and above 4096 tiles, the
            common and the general epilogue branch, under the forced three-per-CU and 384-slot tilings too), the NHWC apply
            (every activation, channel tails, views at c_off > 0, the zeroed padding lanes), the feature-form apply with and
            without the nearest gather, both sos_feat_to_nhwc kernels;
  backward: sos_bn_bwd's three reduce kernels -- the per-wave streaming ReLU reduce (>= 2^20 pixels, <= 64 channel groups,
            16-bit storage), the block-interleaved ReLU reduce, the general reduce (PReLU with its slope gradient, Sigmoid, none,
            the bias + activation mode mean = NULL) -- the finalize's paired loop (nblk > 256), out_scale, dx;
            sos_act_bwd_from_y; train_ops.colsum.

Every case runs in the three storage modes (bf16, fp16, bf16x3) and on two kinds of input:
  exact  : small integers and dyadic fractions for which every sum a kernel can form is exactly representable in f32 (each case
           asserts its bound), so the result does not depend on the order of summation and a dropped or double-counted pixel is
           an exact mismatch: reductions and elementwise outputs are compared for equality, dx within 1 storage ulp;
  random : per-channel means at 0, 1, 4 and 16 standard deviations (the f32 sum of squares in var = q / n - mean^2), dy ~ N(0, 1)
           and dy at the magnitude a loss scale gives it (with out_scale = 1 / scale): elementwise outputs within 1 storage ulp,
           reductions relative to the sum of |terms|.
Each case also asserts that it lands on the launch path it is named for (mirrors of the dispatch conditions of bn.hip)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bn_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SENT = 7.0                  # sentinel of the 16-bit buffers (exact in bf16 and fp16)
SLOPE = 0.25
F32_EVAL = 2.0 ** -22       # allowance of an elementwise output for its f32 evaluation (a few roundings), times the sum of |terms|
MEAN_OFFSETS = (0.0, 1.0, 4.0, 16.0)        # per-channel means of the random inputs, in standard deviations
# random inputs (relative to (|mean| + sigma), to invstd, to the sum of |terms| of the reduction): about 2x the worst value
# observed on MI355X over the cases below in the three modes, each under the ceiling that f32 partials combined in double should
# reach (1e-6, 2e-5, 1e-4, 1e-5).
TOL_MEAN = 1.3e-7           # observed 6.6e-8
TOL_INVSTD = 6e-6           # |mean| <= 4 sigma: observed 3.1e-6
TOL_INVSTD_16 = 9.5e-5      # |mean| = 16 sigma (the cancellation in q / n - mean^2): observed 4.8e-5
TOL_RED = 1.5e-7            # dgamma 7.7e-8, dbeta 4.3e-8, dslope 4.2e-9 observed
LOSS_SCALE = 64.0           # "random-loss-scaled" backward inputs: dy x LOSS_SCALE, out_scale = 1 / LOSS_SCALE
EXACT_OUT_SCALE = 2.0 ** -8  # fp16 exact inputs: a power-of-two out_scale keeps the parameter gradients exact


@pytest.fixture(params=["bf16", "fp16", "bf16x3"])
def mode(request):
    """The kernels' storage modes: bfloat16 and IEEE half (the two library builds) and the three-pass split."""
    import sos_amd
    sos_amd.set_precision(request.param)
    try:
        yield request.param
    finally:
        sos_amd.set_precision("bf16")


def _L():
    from sos_amd import _lib as L
    return L


def _r8(c):
    return (c + 7) // 8 * 8


def _r16(c):
    return (c + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ coverage guard
# Mirrors of the launch choices in csrc/bn.hip; each case asserts the path it is named for, so that a later dispatch change
# cannot silently drop coverage.

def stats_blocks(npix):
    """sos_bn_stats_blocks: one workgroup per 256 pixels, at most BN_MAX_BLOCKS = 2048."""
    want = min(max((npix + 255) // 256, 1), 2048)
    got = _L().lib().sos_bn_stats_blocks(npix)
    assert got == want, (npix, got, want)
    return got


def bwd_reduce_path(npix, C, act, x3):
    """sos_bn_bwd's reduce kernel (`use_stream`): the per-wave streaming kernel for ReLU, 16-bit storage, (C + 7) / 8 <= 64
    channel groups and npix >= 2^20 unless SOS_BN_STREAM=0; else bn_bwd_reduce_kernel<true> (ReLU) or <false>."""
    stream_wgs = int(os.environ.get("SOS_BN_STREAM", "512"))
    if stream_wgs > 0 and act == R.RELU and not x3 and (C + 7) // 8 <= 64 and npix >= 1 << 20:
        return "stream"
    return "relu" if act == R.RELU else "general"


def feat_to_nhwc_path(W, Wo, ranges, x3, C, c_off, row):
    """sos_feat_to_nhwc: the LDS tile kernel for W == Wo, no pooling ranges, 16-bit storage, <= 8 channels in one aligned run."""
    tile = (not ranges and W == Wo and not x3 and C <= 8 and c_off % 8 == 0 and c_off + 8 <= row
            and not os.environ.get("SOS_FEAT_NO_TILE"))
    return "tile" if tile else "general"


# ------------------------------------------------------------------------------------------------ buffers and inputs
class Rows:
    """A 16-bit NHWC activation (engine.Act of npix pixels, thirds hi | hi | lo in bf16x3) pre-filled with SENT."""

    def __init__(self, npix, cs, x3):
        from sos_amd import engine as E
        self.act = E.Act(1, 1, npix, cs, x3, torch.device("cuda"))
        self.act.t.fill_(SENT)
        self.npix, self.cs, self.x3, self.nseg = npix, cs, x3, 3 if x3 else 1
        self.t = self.act.t.view(npix, self.nseg * cs)

    def view(self, c_off, C):
        from sos_amd import engine as E
        return E.view(self.act, c_off, C)

    def put(self, c_off, v):
        """Store f32 [npix, C]: hi = v rounded to the storage type (+ lo = the rest in bf16x3).  Returns the value held (f32,
        exact: hi + lo spans fewer than 24 bits)."""
        C = v.shape[1]
        hi = v.to(self.t.dtype)
        self.t[:, c_off:c_off + C] = hi
        held = hi.float()
        if self.x3:
            lo = (v - held).to(self.t.dtype)
            self.t[:, self.cs + c_off:self.cs + c_off + C] = hi
            self.t[:, 2 * self.cs + c_off:2 * self.cs + c_off + C] = lo
            held = held + lo.float()
        return held

    def third(self, k, c0, c1):
        return self.t[:, k * self.cs + c0:k * self.cs + c1]

    def get(self, c0, c1):
        """The value held in channels [c0, c1): hi (+ lo), float64."""
        v = self.third(0, c0, c1).double()
        if self.x3:
            v = v + self.third(2, c0, c1).double()
        return v

    def check_outside(self, c_off, C, written):
        """Channels [c_off + C, c_off + written) of every third are 0 (the zeroed padding lanes the next conv reads), the hi copy
        equals hi, and everything outside [c_off, c_off + written) still holds SENT."""
        for k in range(self.nseg):
            th = self.t[:, k * self.cs:(k + 1) * self.cs]
            assert bool((th[:, :c_off] == SENT).all()) and bool((th[:, c_off + written:] == SENT).all()), f"third {k}: write outside the view"
            assert bool((th[:, c_off + C:c_off + written] == 0).all()), f"third {k}: padding lanes not zero"
        if self.x3:
            assert torch.equal(self.third(0, c_off, c_off + C), self.third(1, c_off, c_off + C)), "hi copy differs from hi"


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ints(seed, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed), device="cuda", dtype=torch.int32).float()


def _random_x(seed, npix, C, sigma=1.0):
    off = torch.tensor([MEAN_OFFSETS[c % 4] for c in range(C)], device="cuda")
    return (torch.randn((npix, C), generator=_gen(seed), device="cuda") + off) * sigma


def _ulp(v, mode):
    """Storage ulp of `mode` at |v| (float64): bf16 8 significant bits, fp16 11 (spacing 2^-24 below 2^-14); bf16x3 hi + lo:
    lo is the bf16 rounding of a residual of up to half an ulp of hi, and hi may round up into the next binade, so hi + lo
    keeps 16 bits of that binade (an error of up to 2^-15 of |v|'s own binade: observed for dx just below a power of two)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-30)))
    if mode == "fp16":
        return torch.exp2(e.clamp_min(-14) - 10)
    return torch.exp2(e - (7 if mode == "bf16" else 15))


def _f32ulp(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().double().clamp_min(1e-38))) - 23)


def _check_elementwise(mode, got, ref, terms, what):
    """|got - ref| <= 1 storage ulp at ref + F32_EVAL * (sum of |terms| of the f32 evaluation)."""
    err = (got - ref).abs()
    bound = _ulp(ref, mode) + F32_EVAL * terms
    bad = err > bound
    assert not bool(bad.any()), (what, float(err.max()), int(bad.sum()))


def _rel_obs(tag, err, scale):
    """max err / scale (both float64 tensors), printed as an observation for the tolerance constants."""
    r = float((err / scale.clamp_min(1e-300)).max())
    print(f"[bn] {tag}: {r:.2e}")
    return r


# ------------------------------------------------------------------------------------------------ forward: statistics pass
STATS_CASES = [
    # (npix, C, c_off, cs, sos_bn_stats_blocks)
    (7, 10, 0, 16, 1),
    (65436, 48, 0, 48, 256),
    (65537, 100, 0, 112, 257),
    (131065, 96, 0, 96, 512),
    (131073, 2, 0, 16, 513),
    (524288, 256, 0, 256, 2048),            # the cap
    (1093632, 48, 0, 48, 2048),             # 24 x 256 x 178: many strides per lane + the BN_U tail
    (1093632, 100, 0, 112, 2048),
    (1093632, 10, 0, 16, 2048),
    (65537, 48, 16, 96, 257),               # a view at c_off > 0 inside a wider row
]


def _gamma_beta(C, seed):
    g = 1.0 + 0.25 * _ints(seed, (C,), -2, 2)
    b = 0.125 * _ints(seed + 1, (C,), -4, 4)
    return g, b


def _check_finalize_outputs(mode, tag, exact, st, s_sum, count, gamma, beta, mean_k, invstd_k, scale_k, shift_k):
    """mean / invstd / scale / shift of bn_finalize_kernel against the float64 statistics `st` (exact: s_sum is the exact sum)."""
    if exact:
        assert torch.equal(mean_k, (s_sum / count).float()), f"{tag}: save_mean"
        ref_is = st["invstd"].float()
        assert bool(((invstd_k.double() - ref_is.double()).abs() <= _f32ulp(ref_is)).all()), f"{tag}: invstd beyond 1 f32 ulp"
    else:
        sigma = st["var"].sqrt()
        assert _rel_obs(f"{tag} mean", (mean_k.double() - st["mean"]).abs(), st["mean"].abs() + sigma) < TOL_MEAN
        rel = (invstd_k.double() - st["invstd"]).abs() / st["invstd"]
        far = torch.tensor([MEAN_OFFSETS[c % 4] == 16.0 for c in range(len(rel))], device=rel.device)
        if bool((~far).any()):
            assert _rel_obs(f"{tag} invstd (<= 4 sigma)", rel[~far], torch.ones_like(rel[~far])) < TOL_INVSTD
        if bool(far.any()):
            assert _rel_obs(f"{tag} invstd (16 sigma)", rel[far], torch.ones_like(rel[far])) < TOL_INVSTD_16
    # scale and shift from the kernel's own f32 mean / invstd, as the finalize defines them (the shift may be contracted)
    assert torch.equal(scale_k, (gamma.double() * invstd_k.double()).float()), f"{tag}: scale"
    c1 = (beta.double() - (mean_k.double() * scale_k.double()).float().double()).float()
    c2 = (beta.double() - mean_k.double() * scale_k.double()).float()
    assert bool(((shift_k == c1) | (shift_k == c2)).all()), f"{tag}: shift"


def _check_running(tag, exact, rm_prev, rv_prev, rm_k, rv_k, mean_k, st):
    """One running-statistics update from the kernel's previous values (momentum and 1 - momentum as the f32 values)."""
    m = R.MOMENTUM
    keep = float(torch.tensor(1.0 - m, dtype=torch.float32))
    n = st["count"]
    want_m = keep * rm_prev.double() + m * mean_k.double()
    want_v = keep * rv_prev.double() + m * st["var"] * n / max(n - 1, 1)
    # (two f32 products and a sum: 2 ulp of the larger term -- the terms may cancel)
    terms_m = torch.maximum((keep * rm_prev.double()).abs(), (m * mean_k.double()).abs())
    assert bool(((rm_k.double() - want_m).abs() <= 2 * _f32ulp(terms_m) + 1e-45).all()), f"{tag}: running_mean"
    slack = 0.0 if exact else 2.0 * TOL_INVSTD_16 * m * st["var"] * n / max(n - 1, 1)
    assert bool(((rv_k.double() - want_v).abs() <= 2 * _f32ulp(want_v) + slack).all()), f"{tag}: running_var"


@pytest.mark.parametrize("inputs", ["exact", "random"])
@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: f"npix{c[0]}-C{c[1]}-off{c[2]}")
def test_stats_pass_finalize_and_apply(mode, case, inputs):
    """engine.bn_train with the separate statistics pass: two training steps, the saved statistics, the coefficients, the running
    statistics and num_batches_tracked, and the ReLU apply that follows."""
    from sos_amd import engine as E
    npix, C, c_off, cs, blocks = case
    assert stats_blocks(npix) == blocks
    exact = inputs == "exact"
    x3 = mode == "bf16x3"
    raw = Rows(npix, cs, x3)
    dst = Rows(npix, _r16(C) + 16, x3)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    gamma, beta = _gamma_beta(C, 40 + C)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    for step in range(2):
        seed = 1000 * step + npix % 997 + C
        if exact:
            assert 9 * npix < 2 ** 24      # x in {-3..3}: every partial sum of x and x^2 is an integer below 2^24
            v = _ints(seed, (npix, C), -3, 3)
        else:
            v = _random_x(seed, npix, C)
        held = raw.put(c_off, v)
        rm_prev, rv_prev = bn.running_mean.clone(), bn.running_var.clone()
        saved = E.bn_train(raw.act, c_off, C, bn, R.RELU, None, dst.act, 8)
        torch.cuda.synchronize()
        st = R.stats(held, gamma, beta)
        tag = f"stats {mode} {inputs} npix={npix} C={C} step {step + 1}"
        _check_finalize_outputs(mode, tag, exact, st, held.double().sum(0), npix, gamma, beta, saved["mean"], saved["invstd"],
                                saved["scale"], saved["shift"])
        _check_running(tag, exact, rm_prev, rv_prev, bn.running_mean, bn.running_var, saved["mean"], st)
        assert int(bn.num_batches_tracked) == step + 1
        ref = R.apply(held, saved["scale"], saved["shift"], R.RELU)
        terms = (held.double() * saved["scale"].double()).abs() + saved["shift"].double().abs()
        _check_elementwise(mode, dst.get(8, 8 + C), ref, terms, tag + " apply")
        dst.check_outside(8, C, _r8(C))


# ------------------------------------------------------------------------------------------------ forward: finalize alone
# sos_bn_finalize takes bn_finalize_kernel<1024> from 4096 partial rows on and <256> below; the test cannot observe which template
# ran, so the row counts straddle that threshold and each template's 4-way loop (b + 3 * NTH < nblk) and its tail
FIN_NBLK = [1, 255, 256, 257, 4095, 4096, 4097, 12288, 12291]


@pytest.mark.parametrize("count", ["npix", "one"])
@pytest.mark.parametrize("nblk", FIN_NBLK)
def test_finalize_on_synthetic_partials(mode, nblk, count):
    """sos_bn_finalize on f32 partial rows [2][C][nblk] of dyadic values (their float64 sums are exact): count = npix as after a
    statistics pass, count = 1 as in train_ops.colsum (no affine, no running statistics: the "mean" is the plain sum)."""
    L = _L()
    C = 20
    part = torch.empty((2, C, nblk), dtype=torch.float32, device="cuda")
    part[0] = _ints(nblk + 1, (C, nblk), -64, 64) * 0.25
    part[1] = _ints(nblk + 2, (C, nblk), 500, 1000) * 0.25
    S, Q = part[0].double().sum(1), part[1].double().sum(1)     # exact: dyadic values far below 2^53
    scale, shift, mean, invstd = (torch.full((C,), SENT, device="cuda") for _ in range(4))
    if count == "one":
        L.check(L.lib().sos_bn_finalize(L.ptr(part), nblk, C, 1, None, None, 1.0, 0.0, None, None, None, L.ptr(scale), L.ptr(shift),
                                        L.ptr(mean), None, L.stream_ptr()), "sos_bn_finalize")
        torch.cuda.synchronize()
        assert torch.equal(mean, S.float())
        return
    n = 256 * nblk
    gamma, beta = _gamma_beta(C, 7)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    L.check(L.lib().sos_bn_finalize(L.ptr(part), nblk, C, n, L.ptr(gamma), L.ptr(beta), R.EPS, R.MOMENTUM, L.ptr(rm), L.ptr(rv),
                                    L.ptr(nbt), L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd), L.stream_ptr()),
            "sos_bn_finalize")
    torch.cuda.synchronize()
    mu = S / n
    var = (Q / n - mu * mu).clamp_min(0.0)
    st = dict(mean=mu, var=var, invstd=1.0 / torch.sqrt(var + R.EPS), count=n)
    tag = f"finalize {mode} nblk={nblk}"
    _check_finalize_outputs(mode, tag, True, st, S, n, gamma, beta, mean, invstd, scale, shift)
    _check_running(tag, True, torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), rm, rv, mean, st)
    assert int(nbt) == 1


# ------------------------------------------------------------------------------------------------ forward: fused statistics
# (name, cin, cout, (kh, kw), (dil_h, dil_w)): encoder layers of common_nets.make_encoder ('same' zero padding, stride 1) as
# train_ops.encoder_forward_train runs them -- raw output in an Act of cs = round16(cout) channels, cout_store = cs,
# stats_c = cout
FUSED_LAYERS = [
    ("96ch-5x5-dil4x1", 96, 96, (5, 5), (4, 1)),        # the denoiser's encoder_x
    ("48ch-5x5-dil2x2", 48, 48, (5, 5), (2, 2)),        # the detector's encoder / the denoiser's encoder_n
    ("last-1x1-48to4", 48, 4, (1, 1), (1, 1)),          # encoder_n's last block: cout 4, not a multiple of 8, below cs = 16
]
FUSED_H, FUSED_W = 256, 178
FUSED_B = {"below-4096-tiles": 2, "4096-tiles-or-more": 40}     # 40 x 256 x 178 pixels: > 4096 tiles even of 384 slots


@pytest.mark.parametrize("batch", list(FUSED_B))
@pytest.mark.parametrize("layer", FUSED_LAYERS, ids=lambda c: c[0])
def test_fused_stats_from_conv_epilogue(mode, layer, batch):
    """engine.conv_to_act(stats_c=C) -> engine.bn_train(stats=...): the per-tile partial sums the conv epilogue writes (the
    common branch in the 16-bit modes, the general one in bf16x3) and the finalize over them (<1024> from 4096 tiles on) against
    the float64 moments of the raw output READ BACK from the device -- the statistics of what the conv stored, not the conv's
    arithmetic.  Integer input and sparse +-1 weights make every stored output a small integer: each tile's sums are then exact
    in f32 (asserted: max |out|^2 * 384 slots < 2^24) and so is the double sum over the tiles."""
    from sos_amd import engine as E
    name, cin, cout, (kh, kw), dil = layer
    B, H, W = FUSED_B[batch], FUSED_H, FUSED_W
    x3 = mode == "bf16x3"
    dev = torch.device("cuda")
    x = _ints(11 + cin, (B, cin, H, W), -2, 2)
    # weights: 4 taps of +-1 per output channel, the rest 0 (|out| <= 8)
    g = torch.Generator().manual_seed(cout + kh)
    w = torch.zeros(cout, cin * kh * kw)
    for o in range(cout):
        idx = torch.randperm(cin * kh * kw, generator=g)[:4]
        w[o, idx] = torch.randint(0, 2, (4,), generator=g).float() * 2 - 1
    w = w.view(cout, cin, kh, kw).to(dev)
    src = E.pack_input(x, x3)
    cs = _r16(cout)
    raw = E.Act(B, H, W, cs, x3, dev)
    pad = ((kh - 1) // 2 * dil[0], (kw - 1) // 2 * dil[1])
    st = E.conv_to_act(src, 0, src.cs, E.pack_weight(w, src.cs, x3), kh, kw, cout, None, None, R.NONE, raw, cout_store=cs,
                       dil=dil, pad=pad, Ho=H, Wo=W, stats_c=cout)
    partial, tiles = st
    # coverage guard: the tile count conv_to_act returned decides the finalize template (bn_finalize_kernel<1024> from 4096 on)
    assert (tiles >= 4096) == (batch == "4096-tiles-or-more"), tiles
    bn = torch.nn.BatchNorm2d(cout).cuda().train()
    gamma, beta = _gamma_beta(cout, 5)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    y = E.Act(B, H, W, cs, x3, dev)
    saved = E.bn_train(raw, 0, cout, bn, R.RELU, None, y, stats=st)
    torch.cuda.synchronize()
    t = raw.t.view(B * H * W, raw.nseg * cs)
    held = t[:, :cout].double()
    if x3:
        held = held + t[:, 2 * cs:2 * cs + cout].double()
    assert bool((held == held.round()).all()), "conv output not integer"
    assert float(held.abs().max()) ** 2 * 384 < 2 ** 24
    n = B * H * W
    S, Q = held.sum(0), held.square().sum(0)
    tag = f"fused {mode} {name} B={B} tiles={tiles}"
    assert torch.equal(partial[0].double().sum(1), S), f"{tag}: sum of the tile partials"
    assert torch.equal(partial[1].double().sum(1), Q), f"{tag}: sum of squares of the tile partials"
    stats = R.stats(held, gamma, beta)
    _check_finalize_outputs(mode, tag, True, stats, S, n, gamma, beta, saved["mean"], saved["invstd"], saved["scale"],
                            saved["shift"])
    _check_running(tag, True, torch.zeros(cout, device=dev), torch.ones(cout, device=dev), bn.running_mean, bn.running_var,
                   saved["mean"], stats)


@pytest.mark.parametrize("env_kv", [("SOS_CONV_FORCE_W3", "1"), ("SOS_CONV_FORCE_PT3", "1")], ids=["w3", "pt3"])
def test_fused_stats_under_forced_tilings(env_kv):
    """The fused-statistics cases again in a child process with every eligible conv launch forced onto the three-workgroups-per-CU
    kernel (TIGHT epilogue layout: the partial sums go over the walked tile) or onto the 384-slot tiles, spawned the way
    tests/test_gpu_forced_tilings.py spawns its children."""
    env = dict(os.environ, **{env_kv[0]: env_kv[1]})
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_fused_stats_from_conv_epilogue"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ forward: apply
def _dyadic_coefs(C, seed):
    """scale in [-2, 2] step 1/4, shift in [-1, 1] step 1/8: with x in {-3..3}, z and PReLU's z / 4 are exact in bf16 / fp16."""
    return _ints(seed, (C,), -8, 8) * 0.25, _ints(seed + 1, (C,), -8, 8) * 0.125


@pytest.mark.parametrize("inputs", ["exact", "random"])
@pytest.mark.parametrize("kind", [R.NONE, R.RELU, R.PRELU, R.SIGMOID], ids=["none", "relu", "prelu", "sigmoid"])
@pytest.mark.parametrize("C", [10, 48, 100])
def test_apply_nhwc(mode, C, kind, inputs):
    """sos_bn_act_apply through engine.bn_apply with the test's own scale / shift: source at c_off 8, destination at c_off 16 of
    wider rows pre-filled with SENT (also the source's padding channels, which a tail group reads); 200 003 pixels: several
    strides per lane under the 768-workgroup grid."""
    from sos_amd import engine as E
    npix, exact = 200003, inputs == "exact"
    x3 = mode == "bf16x3"
    src, dst = Rows(npix, _r16(C) + 16, x3), Rows(npix, _r16(C) + 32, x3)
    if exact:
        held = src.put(8, _ints(C + kind, (npix, C), -3, 3))
        scale, shift = _dyadic_coefs(C, 3 * C + kind)
    else:
        held = src.put(8, _random_x(C + kind, npix, C))
        scale = (1.0 + 0.5 * torch.randn(C, generator=_gen(C), device="cuda"))
        shift = 0.5 * torch.randn(C, generator=_gen(C + 1), device="cuda")
    slope = torch.full((1,), SLOPE, device="cuda")
    E.bn_apply(src.view(8, C), scale, shift, kind, slope, dst.act, 16, C)
    torch.cuda.synchronize()
    ref = R.apply(held, scale, shift, kind, SLOPE)
    got = dst.get(16, 16 + C)
    if exact and kind != R.SIGMOID:
        assert torch.equal(got, ref), "exact apply differs"
    else:
        terms = (held.double() * scale.double()).abs() + shift.double().abs()
        _check_elementwise(mode, got, ref, terms, f"apply C={C} act={kind}")
    dst.check_outside(16, C, _r8(C))


def _gather(W, Wo):
    from sos_amd import common_nets as CN
    return CN.nearest_index(W, Wo, torch.device("cuda"))


@pytest.mark.parametrize("gather", [False, True], ids=["identity", "gather"])
def test_apply_feature_form(mode, gather):
    """The last encoder block's feature-matrix write (engine.bn_apply(feat=...)): element (b, w', c, h) of the LSTM input
    [B][Wo][row] at (c_off + c) * H + h, read from pixel (b, h, gather[w'], c); exact inputs, index check against a gather of
    the reference; nothing else of the feature rows is touched."""
    from sos_amd import engine as E
    B, H, W, C, c_off = 3, 37, 29, 12, 2
    Wo = 11 if gather else W
    x3 = mode == "bf16x3"
    nseg = 3 if x3 else 1
    src = Rows(B * H * W, 16, x3)
    held = src.put(0, _ints(5, (B * H * W, C), -3, 3))
    scale, shift = _dyadic_coefs(C, 9)
    slope = torch.full((1,), SLOPE, device="cuda")
    nfeat = (c_off + C) * H + 5
    feat = torch.full((B, Wo, nseg * nfeat), SENT, dtype=E.act_dtype(), device="cuda")
    g = _gather(W, Wo) if gather else None
    fd = dict(t=feat, row=nseg * nfeat, third=nfeat, c_off=c_off, H=H, W=W, Wo=Wo, gather=g, x3=x3)
    E.bn_apply(src.view(0, C), scale, shift, R.PRELU, slope, None, 0, C, feat=fd)
    torch.cuda.synchronize()
    ref = R.apply(held, scale, shift, R.PRELU, SLOPE).view(B, H, W, C)
    idx = g.long() if gather else torch.arange(W, device="cuda")
    want = ref[:, :, idx, :].permute(0, 2, 3, 1).reshape(B, Wo, C * H)       # [b][w'][c * H + h]
    lo, hi = c_off * H, (c_off + C) * H
    got = feat[..., lo:hi].double()
    if x3:
        assert torch.equal(feat[..., nfeat + lo:nfeat + hi], feat[..., lo:hi]), "hi copy"
        got = got + feat[..., 2 * nfeat + lo:2 * nfeat + hi].double()
    assert torch.equal(got, want), "feature-form apply differs"
    for k in range(nseg):
        seg = feat[..., k * nfeat:(k + 1) * nfeat]
        assert bool((seg[..., :lo] == SENT).all()) and bool((seg[..., hi:] == SENT).all()), "write outside the feature slice"


@pytest.mark.parametrize("kernel", ["tile", "general"])
def test_feat_to_nhwc(mode, kernel):
    """sos_feat_to_nhwc: dy[b][h][w][c] = sum over i in [lo[w], hi[w]) of dfeat[b][i][(c_off + c) * H + h] (identity without
    ranges).  tile: W == Wo, no ranges, 6 channels, H = 130 (not a multiple of 64), W = 21 (not a multiple of 8) -- the LDS
    tile kernel in the 16-bit modes; general: nearest-gather ranges (W = 13 columns read by Wo = 29), 12 channels; bf16x3 always
    takes the general kernel.  Exact integer inputs; index check against a numpy range sum."""
    from sos_amd import train_ops as TO
    from sos_amd import engine as E
    x3 = mode == "bf16x3"
    nseg = 3 if x3 else 1
    if kernel == "tile":
        B, H, W, Wo, C, fc_off = 2, 130, 21, 21, 6, 1
    else:
        B, H, W, Wo, C, fc_off = 2, 37, 13, 29, 12, 0
    nfeat = (fc_off + C) * H + 3
    f16 = torch.full((B, Wo, nseg * nfeat), SENT, dtype=E.act_dtype(), device="cuda")
    vals = _ints(77, (B, Wo, C * H), -3, 3)
    f16[..., fc_off * H:(fc_off + C) * H] = vals.to(f16.dtype)
    held = vals.double()
    if x3:
        lov = 0.0078125 * _ints(78, (B, Wo, C * H), -3, 3)
        f16[..., 2 * nfeat + fc_off * H:2 * nfeat + (fc_off + C) * H] = lov.to(f16.dtype)
        held = held + lov.double()
    if kernel == "tile":
        lo = hi = None
    else:
        lo_np, hi_np = TO.gather_ranges(_gather(W, Wo).cpu().numpy(), W)
        assert int((hi_np - lo_np).max()) > 1          # columns summed over more than one feature row
        lo, hi = torch.from_numpy(lo_np).cuda(), torch.from_numpy(hi_np).cuda()
    out = Rows(B * H * W, 16, x3)
    ov = out.view(0, C)
    assert feat_to_nhwc_path(W, Wo, lo is not None, x3, C, 0, ov.row) == ("general" if x3 else kernel)
    fv = _L().View()
    fv.ptr, fv.npix, fv.row, fv.c_off, fv.C, fv.x3, fv.third = f16.data_ptr(), 1, nseg * nfeat, fc_off, C, int(x3), nfeat
    L = _L()
    L.check(L.lib().sos_feat_to_nhwc(ctypes.byref(fv), B, H, W, Wo, L.ptr(lo), L.ptr(hi), ctypes.byref(ov), L.stream_ptr()),
            "sos_feat_to_nhwc")
    torch.cuda.synchronize()
    h = held.cpu().numpy().reshape(B, Wo, C, H)
    want = np.zeros((B, H, W, C))
    for w in range(W):
        i0, i1 = (w, w + 1) if lo is None else (int(lo_np[w]), int(hi_np[w]))
        want[:, :, w, :] = h[:, i0:i1].sum(axis=1).transpose(0, 2, 1)
    got = out.get(0, C).cpu().numpy().reshape(B, H, W, C)
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    out.check_outside(0, C, 8 if C <= 8 else C)


# ------------------------------------------------------------------------------------------------ backward
def _bn_bwd(dyv, xv, scale, shift, mean, invstd, gamma, kind, slope, dxv, out_scale, C, npix):
    """sos_bn_bwd by ctypes: (dgamma, dbeta, dslope, coef [4][C])."""
    L = _L()
    nblk = stats_blocks(npix)
    partial = torch.empty((3, C, nblk), dtype=torch.float32, device="cuda")
    coef = torch.empty((4, C), dtype=torch.float32, device="cuda")
    dgamma, dbeta = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dslope = torch.empty(1, device="cuda") if slope is not None else None
    L.check(L.lib().sos_bn_bwd(ctypes.byref(dyv), ctypes.byref(xv), L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd),
                               L.ptr(gamma), kind, L.ptr(slope), L.ptr(partial), L.ptr(coef), L.ptr(dgamma), L.ptr(dbeta),
                               L.ptr(dslope), ctypes.byref(dxv), L.ptr(out_scale), L.stream_ptr()), "sos_bn_bwd")
    torch.cuda.synchronize()
    return dgamma, dbeta, dslope, coef


def _run_bwd(mode, npix, C, kind, inputs, path, no_bn=False, chunk=128):
    """One sos_bn_bwd call on x (c_off 8), dy (c_off 0) and dx (c_off 16) in rows of three different widths; the reference is
    evaluated in channel chunks on the device."""
    x3 = mode == "bf16x3"
    assert bwd_reduce_path(npix, C, kind, x3) == path, (npix, C, kind, x3, path)
    exact = inputs == "exact"
    X, DY, DX = Rows(npix, _r16(C) + 16, x3), Rows(npix, _r16(C), x3), Rows(npix, _r16(C) + 32, x3)
    seed = npix % 1009 + 7 * C + kind
    if exact:
        # x, dy in {-2..2}, integer mean, power-of-two invstd / gamma / scale, shift 1/4 (z is never 0), slope 1/4
        xs, dys = _ints(seed, (npix, C), -2, 2), _ints(seed + 1, (npix, C), -2, 2)
        mean = _ints(seed + 2, (C,), -1, 1)
        invstd = torch.full((C,), 0.5, device="cuda")
        gamma = torch.exp2(_ints(seed + 3, (C,), 0, 2))
        scale, shift = gamma * invstd, torch.full((C,), 0.25, device="cuda")
        os_ = EXACT_OUT_SCALE if mode == "fp16" else 1.0
    else:
        xs = _random_x(seed, npix, C)
        dys = torch.randn((npix, C), generator=_gen(seed + 1), device="cuda")
        os_ = 1.0
        if inputs == "random-loss-scaled":
            dys, os_ = dys * LOSS_SCALE, 1.0 / LOSS_SCALE
    held_x, held_dy = X.put(8, xs), DY.put(0, dys)
    if not exact:
        gamma = 1.0 + 0.25 * torch.randn(C, generator=_gen(seed + 4), device="cuda")
        st = R.stats(held_x, gamma, 0.1 * torch.randn(C, generator=_gen(seed + 5), device="cuda"))
        mean, invstd, scale, shift = (st[k].float() for k in ("mean", "invstd", "scale", "shift"))
    del xs, dys
    slope = torch.full((1,), SLOPE, device="cuda") if kind == R.PRELU else None
    out_scale = torch.full((1,), os_, device="cuda") if os_ != 1.0 else None
    dgamma, dbeta, dslope, coef = _bn_bwd(DY.view(0, C), X.view(8, C), scale, shift, None if no_bn else mean,
                                          None if no_bn else invstd, gamma, kind, slope, DX.view(16, C), out_scale, C, npix)
    tag = f"bwd {path} {mode} {inputs} npix={npix} C={C} act={kind}{' no-bn' if no_bn else ''}"
    s3_sum, t3_sum = 0.0, 0.0
    for c0 in range(0, C, chunk):
        c1 = min(C, c0 + chunk)
        sl = slice(c0, c1)
        ref = R.backward(held_x[:, sl], held_dy[:, sl], scale[sl], shift[sl], None if no_bn else mean[sl],
                         None if no_bn else invstd[sl], gamma[sl], kind, SLOPE, os_)
        s3_sum, t3_sum = s3_sum + ref["dslope"], t3_sum + float(ref["t3"].sum()) * os_
        got_dx = DX.get(16 + c0, 16 + c1)
        if exact and kind != R.SIGMOID:        # (a Sigmoid's derivative is not exact: the tolerance checks below)
            # every sum of the reduce is a multiple of its granularity below 2^24 of them: exact in f32 in any order
            g1 = 0.25 if kind == R.PRELU else 1.0
            g2 = g1 * (1.0 if no_bn else 0.5)
            assert float(ref["t1"].max()) / g1 < 2 ** 24 and float(ref["t2"].max()) / g2 < 2 ** 24
            if kind == R.PRELU:
                assert float(ref["t3"].max()) / 0.25 < 2 ** 24       # z on a 1/4 grid
            assert torch.equal(dgamma[sl], ref["dgamma"].float()), f"{tag}: dgamma"
            assert torch.equal(dbeta[sl], ref["dbeta"].float()), f"{tag}: dbeta"
            _check_elementwise(mode, got_dx, ref["dx"], ref["dx_terms"], tag + " dx")
        else:
            _rel_obs(tag + " dgamma", (dgamma[sl].double() - ref["dgamma"]).abs(), ref["t2"] * os_)
            _rel_obs(tag + " dbeta", (dbeta[sl].double() - ref["dbeta"]).abs(), ref["t1"] * os_)
            assert bool(((dgamma[sl].double() - ref["dgamma"]).abs() <= TOL_RED * ref["t2"] * os_ + 1e-30).all()), f"{tag}: dgamma"
            assert bool(((dbeta[sl].double() - ref["dbeta"]).abs() <= TOL_RED * ref["t1"] * os_ + 1e-30).all()), f"{tag}: dbeta"
            # dx from the kernel's own coefficients a, b, c (checked against the exact ones here) within 1 storage ulp
            a, b, c = (coef[k, sl].double() for k in range(3))
            n = npix
            if no_bn:
                assert bool((coef[0, sl] == 1).all() and (coef[1, sl] == 0).all() and (coef[2, sl] == 0).all()), f"{tag}: (a, b, c)"
            else:
                assert torch.equal(coef[0, sl], ref["a"].float()), f"{tag}: a"
                assert bool(((b - ref["b"]).abs() <= ref["a"].abs() * TOL_RED * ref["t2"] / n + _f32ulp(ref["b"])).all()), f"{tag}: b"
                assert bool(((c - ref["c"]).abs() <= ref["a"].abs() * TOL_RED * ref["t1"] / n + _f32ulp(ref["c"])).all()), f"{tag}: c"
            xh = held_x[:, sl].double() if no_bn else (held_x[:, sl].double() - mean[sl].double()) * invstd[sl].double()
            z = held_x[:, sl].double() * scale[sl].double() + shift[sl].double()
            dz = held_dy[:, sl].double() * R.act_grad(z, kind, SLOPE)
            want = a * dz + b * xh + c
            terms = (a * dz).abs() + (b * xh).abs() + c.abs()
            if kind == R.SIGMOID:       # y (1 - y) in f32: an absolute error of a few 2^-24 where y is near 1
                terms = terms + (a * held_dy[:, sl].double()).abs()
            _check_elementwise(mode, got_dx, want, terms, tag + " dx")
        del ref, got_dx
    if kind == R.PRELU:
        if exact:
            assert float(dslope) == float(torch.as_tensor(s3_sum).float()), f"{tag}: dslope"      # (PReLU: exact inputs)
        else:
            _rel_obs(tag + " dslope", torch.tensor(abs(float(dslope) - float(s3_sum)), dtype=torch.float64),
                     torch.tensor(t3_sum, dtype=torch.float64))
            assert abs(float(dslope) - float(s3_sum)) <= TOL_RED * t3_sum, f"{tag}: dslope"
    DX.check_outside(16, C, _r8(C))


# random inputs: dy ~ N(0, 1) with out_scale 1, and dy at the magnitude a loss scale gives it in fp16 (x LOSS_SCALE, out_scale =
# 1 / LOSS_SCALE; the ABI takes out_scale in every mode)
BWD_INPUTS = ["exact", "random", "random-loss-scaled"]
BIG = [1 << 20, 1093632, (1 << 20) + 4097]
STREAM_CASES = [(BIG[0], 8), (BIG[0], 48), (BIG[0], 96), (BIG[0], 100), (BIG[0], 512), (BIG[1], 48), (BIG[1], 100),
                (BIG[2], 8), (BIG[2], 96), (BIG[2], 512)]


@pytest.mark.parametrize("inputs", BWD_INPUTS)
@pytest.mark.parametrize("npix,C", STREAM_CASES)
def test_bwd_relu_full_resolution(mode, npix, C, inputs):
    """The full-resolution ReLU blocks: the per-wave streaming reduce in the 16-bit modes (C = 8: one channel group, 100: a partial
    tail group and idle lanes, 512: 64 groups), the block-interleaved ReLU reduce in bf16x3."""
    _run_bwd(mode, npix, C, R.RELU, inputs, "relu" if mode == "bf16x3" else "stream")


@pytest.mark.parametrize("inputs", BWD_INPUTS)
@pytest.mark.parametrize("npix,C", [((1 << 20) - 1, 48), ((1 << 20) - 1, 100), (1 << 20, 520)])
def test_bwd_relu_block_interleaved(mode, npix, C, inputs):
    """bn_bwd_reduce_kernel<true> at the edges of the streaming kernel's domain: one pixel short of 2^20, and 520 channels (65
    groups, the first width past 64) at 2^20."""
    _run_bwd(mode, npix, C, R.RELU, inputs, "relu")


GENERAL_CASES = [
    # (npix, C, act, no_bn)                      sos_bn_stats_blocks
    (200, 64, R.PRELU, False),                   # 1
    (65436, 100, R.PRELU, False),                # 256
    (65537, 64, R.PRELU, False),                 # 257: the finalize's paired loop + one
    (131065, 256, R.PRELU, False),               # 512
    (131073, 100, R.PRELU, False),               # 513
    (524288, 64, R.PRELU, False),                # 2048
    (65537, 48, R.SIGMOID, False),
    (131073, 40, R.NONE, False),
    (513, 24, R.NONE, True),                     # the bias + activation mode (mean = NULL)
    (131073, 100, R.PRELU, True),
    (524288, 48, R.RELU, True),
]


@pytest.mark.parametrize("inputs", BWD_INPUTS)
@pytest.mark.parametrize("case", GENERAL_CASES, ids=lambda c: f"npix{c[0]}-C{c[1]}-act{c[2]}{'-nobn' if c[3] else ''}")
def test_bwd_general(mode, case, inputs):
    """The U-Net's PReLU layers (the slope gradient S3 and slope_sum_kernel), the ABI-only modes (Sigmoid, none, mean = NULL),
    out_scale != 1 in fp16, and partial-row counts 1 .. 2048 for bn_bwd_finalize_kernel's paired loop."""
    npix, C, kind, no_bn = case
    _run_bwd(mode, npix, C, kind, inputs, "relu" if kind == R.RELU else "general", no_bn=no_bn)


def test_exact_cases_with_small_grids():
    """The exact-input cases again in a child process with SOS_BN_STREAM=7 (seven streaming workgroups: long per-wave runs with
    odd iteration counts of the two-register-set loop) and SOS_BN_GRID=3 (apply passes that walk many strides)."""
    env = dict(os.environ, SOS_BN_STREAM="7", SOS_BN_GRID="3")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "not random and not small_grids"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ small companions
@pytest.mark.parametrize("kind", [R.RELU, R.SIGMOID, R.NONE], ids=["relu", "sigmoid", "none"])
def test_act_bwd_from_y(mode, kind):
    """sos_act_bwd_from_y: dz = dy * act'(y) from the layer's output: ReLU exactly, Sigmoid within 1 ulp, none exactly; padding
    lanes zero."""
    from sos_amd import train_ops as TO
    npix, C = 50001, 20
    x3 = mode == "bf16x3"
    Y, DY, DZ = Rows(npix, 32, x3), Rows(npix, 32, x3), Rows(npix, 32, x3)
    if kind == R.SIGMOID:
        y = Y.put(0, torch.rand((npix, C), generator=_gen(3), device="cuda"))
    else:
        y = Y.put(0, 0.25 * _ints(3, (npix, C), -4, 4))
    dy = DY.put(0, _ints(4, (npix, C), -3, 3))
    TO.act_bwd_from_y(DY.act, Y.act, kind, DZ.act, C)
    torch.cuda.synchronize()
    got = DZ.get(0, C)
    if kind == R.RELU:
        assert torch.equal(got, torch.where(y > 0, dy, torch.zeros_like(dy)).double())
    elif kind == R.NONE:
        assert torch.equal(got, dy.double())
    else:
        want = dy.double() * y.double() * (1.0 - y.double())
        _check_elementwise(mode, got, want, want.abs() + dy.double().abs() * y.double(), "sigmoid from y")
    DZ.check_outside(0, C, _r8(C))


def test_colsum(mode):
    """train_ops.colsum (sos_bn_stats + sos_bn_finalize with count = 1): exact column sums of integers, divided by the
    power-of-two loss scale in fp16."""
    from sos_amd import engine as E, train_ops as TO
    npix, C, c_off = 300001, 40, 8
    x3 = mode == "bf16x3"
    A = Rows(npix, 64, x3)
    held = A.put(c_off, _ints(8, (npix, C), -2, 2))
    assert 2 * npix < 2 ** 24
    g = torch.ones(4, device="cuda")
    with E.backward_scale(g) as gs:
        out = TO.colsum(A.act, c_off, C)
    torch.cuda.synchronize()
    inv = 1.0 if gs.inv is None else float(gs.inv)
    if mode == "fp16":
        assert inv < 1.0 and np.log2(inv) == int(np.log2(inv)), inv
    assert torch.equal(out, (held.double().sum(0) * inv).float())
