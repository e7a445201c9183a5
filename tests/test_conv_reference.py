"""tests/conv_reference.py (the float64 reference of sos_conv2d_fwd that tests/test_gpu_conv_tilings.py compares the kernels with)
against an independent formulation -- torch.nn.functional.conv2d in float64 on an explicitly padded NCHW input -- for every
padding / stride / dilation combination of the GPU tests, the ragged semantics on a hand-made two-clip batch, the three products of
the bf16x3 mode, the column gather, the fused input BatchNorm, the epilogue, accumulation and the statistics; and the input
generators against the exactness conditions the reference asserts.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import conv_pin as P
import conv_reference as R

MODES = ["bf16", "bf16x3", "fp16"]
GEOMETRIES = {(s.k, s.dil, s.stride, s.reflect): s for s in P.ALL_SHAPES}


def build_case(s, mode, idx=0, cin=None, cout=None, gen=(R.exact_input, R.exact_weight), **kw):
    """Case + the logical (B, H, W, C) input and (O, I, kh, kw) weight it was packed from."""
    cin = s.cin if cin is None else cin
    cout = s.cout if cout is None else cout
    x = gen[0](100 + idx, (s.B, s.H, s.W, cin), mode)
    w = gen[1](200 + idx, (cout, cin, s.k[0], s.k[1]), mode)
    nseg = 3 if mode == "bf16x3" else 1
    c = R.Case(inp=R.pack_input(x, cin, mode), wgt=R.pack_weight(w, cin, mode), cin=cin, cout=cout, kh=s.k[0], kw=s.k[1], Ho=s.Ho, Wo=s.Wo,
               in_nseg=nseg, in_seg_stride=cin, stride=s.stride, dil_h=s.dil[0], dil_w=s.dil[1], pad_top=s.pad[0], pad_left=s.pad[1],
               pad_mode=R.REFLECT if s.reflect else R.ZERO, **kw)
    return c, x, w


def conv2d(x, w, s, Ho, Wo):
    """F.conv2d in float64 of (B, H, W, C) by (O, I, kh, kw) on an explicitly padded input -> (B, Ho, Wo, O)."""
    xn = x.permute(0, 3, 1, 2)
    ph, pw = s.pad
    # (bottom / right padding: whatever the last output row / column reaches)
    eh = max(0, (Ho - 1) * s.stride - ph + (s.k[0] - 1) * s.dil[0] - (s.H - 1))
    ew = max(0, (Wo - 1) * s.stride - pw + (s.k[1] - 1) * s.dil[1] - (x.shape[2] - 1))
    xp = F.pad(xn, (pw, ew, ph, eh), mode="reflect" if s.reflect else "constant")
    y = F.conv2d(xp, w, None, s.stride, 0, s.dil)
    return y[:, :, :Ho, :Wo].permute(0, 2, 3, 1)


def three_products(x, w, mode, s, Ho, Wo):
    if mode != "bf16x3":
        return conv2d(x, w, s, Ho, Wo)
    xh, xl = R.split_storage(x, mode)
    wh, wl = R.split_storage(w, mode)
    return conv2d(xh, wh, s, Ho, Wo) + conv2d(xh, wl, s, Ho, Wo) + conv2d(xl, wh, s, Ho, Wo)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", sorted(GEOMETRIES), ids=lambda g: f"k{g[0][0]}x{g[0][1]}-d{g[1][0]}x{g[1][1]}-s{g[2]}-{'reflect' if g[3] else 'zero'}")
def test_contraction_equals_conv2d_on_padded_input(geom, mode):
    """Every (kernel, dilation, stride, padding) of the GPU tests, at its own image size, 32 -> 40 channels: the contraction of the
    exact inputs equals F.conv2d on the padded input bit for bit (all sums are exact in float64), and the case passes the
    reference's own exactness assertions."""
    s = GEOMETRIES[geom]
    c, x, w = build_case(s, mode, cin=32, cout=40)
    r = R.reference(c, mode)
    assert torch.equal(r.acc, three_products(x, w, mode, s, s.Ho, s.Wo))
    assert r.n_terms == s.k[0] * s.k[1] * (3 if mode == "bf16x3" else 1) * 32
    assert float(r.acc.abs().max()) > 8          # (not a degenerate case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", P.ALL_SHAPES, ids=lambda s: s.name)
def test_every_gpu_shape_is_an_exact_case(s, mode):
    """The exact inputs of every shape of tests/test_gpu_conv_tilings.py at its full channel counts satisfy the conditions the
    reference asserts: storage-representable values, sums of |terms| below 2^(24 - q), an exact epilogue."""
    scale, shift = R.exact_epilogue(s.cout_pad)
    c, _, _ = build_case(s, mode, scale=scale, shift=shift, act=R.PRELU, slope=0.25)
    r = R.reference(c, mode)
    assert r.q == (9 if mode == "bf16x3" else 0)
    assert float(r.abs_terms.max()) < 2.0 ** (24 - r.q)
    hi, lo = R.stored(c, r, mode)
    assert bool((hi != r.y).any()), "no output needs rounding: the 16-bit comparison would not see the rounding mode"


def test_an_inexact_case_is_refused():
    s = P.ALL_SHAPES[0]
    c, _, _ = build_case(s, "bf16", cin=16, cout=8)
    c.wgt = c.wgt / 3.0
    with pytest.raises(AssertionError):
        R.reference(c, "bf16")
    c, _, _ = build_case(s, "bf16", cin=16, cout=8)
    c.inp = c.inp * 2.0 ** 20                    # representable, but the sums leave 24 bits
    c.wgt = c.wgt + 2.0 ** -7 * (c.wgt != 0)
    with pytest.raises(AssertionError):
        R.reference(c, "bf16")
    c, _, _ = build_case(s, "bf16", cin=16, cout=8, scale=torch.full((32,), 1.0 / 3, dtype=torch.float64), shift=torch.zeros(32, dtype=torch.float64))
    with pytest.raises(AssertionError):
        R.reference(c, "bf16")


def test_bf16x3_forms_three_products_in_pack_weight_order():
    """The packed weight is [w_hi | w_lo | w_hi] against activations [x_hi | x_hi | x_lo] (engine.pack_weight): the reference's
    contraction is x_hi w_hi + x_hi w_lo + x_lo w_hi and differs from the full product by exactly the x_lo w_lo term."""
    from sos_amd import engine as E
    import sos_amd
    s = GEOMETRIES[((5, 5), (2, 3), 1, False)]
    c, x, w = build_case(s, "bf16x3", cin=16, cout=24)
    sos_amd.set_precision("bf16x3")
    try:
        wp = E.pack_weight(w.permute(0, 1, 2, 3).float(), 16, True)
    finally:
        sos_amd.set_precision("bf16")
    assert torch.equal(wp.double(), c.wgt)
    xh, xl = R.split_storage(x, "bf16x3")
    wh, wl = R.split_storage(w, "bf16x3")
    assert bool((xl != 0).any()) and bool((wl != 0).any()) and torch.equal(xh + xl, x) and torch.equal(wh + wl, w)
    r = R.reference(c, "bf16x3")
    full = conv2d(x, w, s, s.Ho, s.Wo)
    assert torch.equal(full - r.acc, conv2d(xl, wl, s, s.Ho, s.Wo)) and bool((full != r.acc).any())


@pytest.mark.parametrize("reflect", [False, True], ids=["zero", "reflect"])
def test_ragged_batch_is_each_clip_at_its_own_width(reflect):
    """Two clips of 9 and 4 columns in a buffer 9 wide, 3x3 taps at dilation (1, 2): every image's border is taken at ITS end (so
    clip 1 equals the convolution of its own 4 columns alone, whatever the buffer holds beyond them) and the columns past
    wo_tab[b] are not written."""
    s = P.Shape("ragged", 16, 8, (3, 3), (1, 2), reflect=reflect, H=5, W=9)
    widths = [9, 4]
    c, x, w = build_case(s, "bf16", wl_tab=widths, wo_tab=widths)
    r = R.reference(c, "bf16")
    assert r.valid.tolist() == [[True] * 9, [True] * 4 + [False] * 5]
    for b, wb in enumerate(widths):
        alone = conv2d(x[b:b + 1, :, :wb], w, s, s.Ho, wb)
        assert torch.equal(r.acc[b, :, :wb], alone[0])
    assert bool((r.acc[1, :, 4:] == 0).all())
    # the hand-made corner: output (row 0, column 3) of clip 1, channel o, zero padding -- the tap at column 3 + 2 lies outside the clip
    if not reflect:
        want = sum(float(w[0, ci, a, t]) * float(x[1, 0 - 1 + a, 3 - 2 + 2 * t, ci])
                   for ci in range(16) for a in (1, 2) for t in (0, 1))
        assert float(r.acc[1, 0, 3, 0]) == want


def test_gather_and_input_batchnorm_and_channel_offset():
    s = P.Shape("g", 16, 8, (3, 3), (1, 1), H=6, W=7)
    g = torch.tensor([0, 0, 1, 2, 2, 3, 4, 4, 5, 6, 6])          # 11 logical columns out of 7 physical ones (nearest resize)
    sg = P.Shape("g", 16, 8, (3, 3), (1, 1), H=6, W=11)
    c, x, w = build_case(s, "fp16", w_gather=g)
    c.Wo = 11
    r = R.reference(c, "fp16")
    assert torch.equal(r.acc, conv2d(x[:, :, g], w, sg, 6, 11))
    # fused input BatchNorm + ReLU = the plain conv of the activated, storage-rounded tensor; zero padding stays zero
    sc = 2.0 ** -(torch.arange(16) % 2).double()
    sh = ((torch.arange(16) % 3).double() - 1) / 64 + 1
    c2, x2, w2 = build_case(s, "bf16", in_scale=sc, in_shift=sh)
    act = R.round_storage((x2 * sc + sh).clamp_min(0), "bf16")
    assert bool((act != (x2 * sc + sh).clamp_min(0)).any())     # (the rounding is visible)
    assert torch.equal(R.reference(c2, "bf16").acc, conv2d(act, w2, s, 6, 7))
    # a channel range inside a wider pixel: the other channels hold 3 and are not read
    for mode in MODES:
        c3, x3, w3 = build_case(s, mode)
        c3.inp = R.pack_input(x3, 48, mode, cin_off=24, fill=3.0)
        c3.cin_off, c3.in_seg_stride = 24, 48
        assert torch.equal(R.reference(c3, mode).acc, three_products(x3, w3, mode, s, 6, 7))


@pytest.mark.parametrize("mode", MODES)
def test_epilogue_rounding_accumulation_and_statistics(mode):
    s = P.Shape("e", 32, 21, (3, 3), (1, 1), reflect=True, H=9, W=11)
    scale, shift = R.exact_epilogue(32)
    for act in (R.NONE, R.RELU, R.PRELU, R.SIGMOID):
        c, x, w = build_case(s, mode, scale=scale, shift=shift, act=act, slope=0.25, cout_store=24)
        r = R.reference(c, mode)
        z = three_products(x, w, mode, s, 9, 11) * scale[:21] + shift[:21]
        want = {R.NONE: z, R.RELU: F.relu(z), R.PRELU: F.prelu(z, torch.tensor([0.25], dtype=torch.float64)), R.SIGMOID: torch.sigmoid(z)}[act]
        assert torch.equal(r.y[..., :21], want) and bool((r.y[..., 21:] == 0).all()) and r.y.shape[-1] == 24
    c, x, w = build_case(s, mode, scale=scale, shift=shift, act=R.RELU, cout_store=24)
    r = R.reference(c, mode)
    hi, lo = R.stored(c, r, mode)
    st = R.storage_dtype(mode)
    assert torch.equal(hi, r.y.float().to(st).double())
    if mode == "bf16x3":
        assert torch.equal(lo, (r.y.float() - hi.float()).to(st).double()) and bool((lo != 0).any())
    else:
        assert lo is None
    assert torch.equal(R.stored(c, r, mode, out="f32").double(), r.y)
    # accumulation: old + the ROUNDED result, rounded again
    c.prev = R._hash_int(7, (s.B, 9, 11, 24), -8, 8).double() / 2
    ah, al = R.stored(c, r, mode)
    tot = hi + (lo if lo is not None else 0) + c.prev
    assert torch.equal(ah, tot.float().to(st).double())
    # statistics of the stored output, through an independent per-channel loop
    c4, _, _ = build_case(s, mode, gen=(R.stats_input, R.stats_weight), scale=R.stats_epilogue(32)[0], shift=R.stats_epilogue(32)[1], act=R.RELU, cout_store=24, stats_c=21)
    r4 = R.reference(c4, mode)
    got = R.statistics(c4, r4, mode)
    h4, l4 = R.stored(c4, r4, mode)
    v = h4 if l4 is None else h4 + l4
    for ch in (0, 7, 20):
        assert float(got[0, ch]) == float(v[..., ch].sum()) and float(got[1, ch]) == float((v[..., ch] ** 2).sum())
    assert bool((got[1] > 0).all())
    if mode == "bf16x3":                         # all three channel segments carry signal in the statistics inputs too
        assert bool((c4.inp[..., 2 * 32:] != 0).any()) and bool((c4.wgt[..., 32:64] != 0).any())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", P.FEATURE_SHAPES, ids=lambda s: s.name)
def test_statistics_generators_sum_exactly_over_a_tile(s, mode):
    scale, shift = R.stats_epilogue(s.cout_pad)
    c, _, _ = build_case(s, mode, gen=(R.stats_input, R.stats_weight), scale=scale, shift=shift, act=R.RELU, stats_c=s.cout)
    r = R.reference(c, mode)
    st = R.statistics(c, r, mode)               # asserts 384 max|v| < 2^(24 - s) and 384 max v^2 < 2^(24 - 2 s)
    assert st.shape == (2, s.cout) and bool((st[1] > 0).all())
