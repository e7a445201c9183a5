"""CPU pin of tests/glue_reference.py (the float64 references of the video glue, crop, fold and gradient-pack kernels' GPU tests)
against torch in float64, and the proof that the shapes of tests/test_gpu_glue.py can tell right from wrong: every wrong kernel
listed below, computed in float64 at the exact shapes and inputs of the GPU tests (tests/glue_cases.py), differs from the
reference by more than the GPU tests' tolerance in at least one storage mode and one listed shape -- the GPU tests do not pass by
slack."""
import pytest
import torch
import torch.nn.functional as F

import glue_cases as K
import glue_reference as R

TOL = 1e-12


def _close(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)
    assert err < TOL, (what, err)


def _rand(seed, *shape):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


STACK_GEOMS = [(B, T, HW, C, kt, out_cs) for B, T, HW, C, _, kt, out_cs in K.STACK_CASES]


# ------------------------------------------------------------------------------------------------ storage model
def test_store_rounds_once_to_nearest_even():
    for mode, dt, bits in (("bf16", torch.bfloat16, 8), ("fp16", torch.float16, 11)):
        v = _rand(1, 4096).float()
        assert torch.equal(R.store(v, mode), v.to(dt).double())
        assert torch.equal(R.split(v, mode), v.to(dt).view(torch.int16))
        # just above a tie of the 16-bit type, by less than f32 resolves: rounding to f32 first would land on the tie and go to even
        ulp = 2.0 ** (1 - bits)
        d = torch.tensor([1.0 + ulp / 2 + 2.0 ** -40, 1.0 + ulp / 2, 1.0 + 3 * ulp / 2, -(1.0 + ulp / 2 + 2.0 ** -40)],
                         dtype=torch.float64)
        assert R.store(d, mode).tolist() == [1.0 + ulp, 1.0, 1.0 + 2 * ulp, -(1.0 + ulp)]
    # IEEE half: subnormals at spacing 2^-24, overflow to infinity
    assert R.store(torch.tensor([2.0 ** -24 * 2.6, 2.0 ** -26, 70000.0]), "fp16").tolist() == [2.0 ** -24 * 3, 0.0, float("inf")]


def test_three_pass_store_holds_hi_plus_lo():
    v = _rand(2, 4096).float()
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    want = hi.double() + lo.double()
    assert torch.equal(R.store(v, "bf16x3"), want)
    b = R.split(v, "bf16x3")
    assert b.shape == (3 * 4096,)
    assert torch.equal(b[:4096], hi.view(torch.int16)) and torch.equal(b[4096:8192], b[:4096])
    assert torch.equal(b[8192:], lo.view(torch.int16))
    assert torch.equal(R.held(b, "bf16x3"), want)
    assert float(((want - v.double()).abs() / v.double().abs()).max()) <= R.UNIT["bf16x3"]
    # a stored value is a fixed point of the split after one more store (what the GPU tests put into their buffers)
    h1 = R.store(want, "bf16x3")
    assert torch.equal(h1, want) and torch.equal(R.split(R.store(h1, "bf16x3"), "bf16x3"), R.split(h1, "bf16x3"))


# ------------------------------------------------------------------------------------------------ the references against torch
@pytest.mark.parametrize("geom", STACK_GEOMS, ids=str)
def test_time_stack_is_pad_along_time_plus_unfold(geom):
    B, T, HW, C, kt, out_cs = geom
    x = _rand(3, B, T, HW, C)
    pt = (kt - 1) // 2
    win = F.pad(x, (0, 0, 0, 0, pt, pt)).unfold(1, kt, 1)              # [B, T, HW, C, kt]
    want = win.permute(0, 1, 2, 4, 3).reshape(B, T, HW, kt * C)
    got = R.time_stack(x, kt, out_cs)
    assert got.shape == (B, T, HW, out_cs)
    _close(got[..., :kt * C], want, "time_stack")
    assert not got[..., kt * C:].any()


@pytest.mark.parametrize("geom", [(2, 5, 3, 4, 3, 5), (2, 2, 3, 4, 3, 5), (2, 4, 2, 3, 6, 3)], ids=str)
def test_conv3d_equals_conv2d_over_the_time_stack(geom):
    B, T, H, W, C, kt = geom
    O = 5
    x = _rand(4, B, C, T, H, W)
    w = _rand(5, O, C, kt, 3, 3)
    want = F.conv3d(x, w, padding=((kt - 1) // 2, 1, 1))               # [B, O, T, H, W]
    rows = x.permute(0, 2, 3, 4, 1).reshape(B, T, H * W, C)
    st = R.time_stack(rows, kt, kt * C + 3)                            # (+ 3 zero padding channels with zero weights)
    w2 = torch.zeros(O, kt * C + 3, 3, 3, dtype=torch.float64)
    w2[:, :kt * C] = w.permute(0, 2, 1, 3, 4).reshape(O, kt * C, 3, 3)
    got = F.conv2d(st.reshape(B * T, H, W, -1).permute(0, 3, 1, 2), w2, padding=1)
    _close(got.reshape(B, T, O, H, W).permute(0, 2, 1, 3, 4), want, "conv over the stack")


@pytest.mark.parametrize("geom", STACK_GEOMS, ids=str)
def test_time_unstack_is_the_transpose_of_time_stack(geom):
    B, T, HW, C, kt, out_cs = geom
    x = _rand(6, B, T, HW, C).requires_grad_()
    d = _rand(7, B, T, HW, out_cs)                                     # non-zero in the padding channels too
    (R.time_stack(x, kt, out_cs) * d).sum().backward()
    got = R.time_unstack(d, C, kt, C + 8)
    _close(got[..., :C], x.grad, "time_unstack")
    assert not got[..., C:].any()
    _close(R.time_unstack_abs(d, C, kt, C), R.time_unstack(d.abs(), C, kt, C), "sum of |terms|")


def test_spatial_mean_and_its_backward():
    x = _rand(8, 3, 49, 5).requires_grad_()
    m = R.spatial_mean(x)
    _close(m.detach(), x.detach().mean(1), "spatial_mean")
    d = _rand(9, 3, 5)
    (m * d).sum().backward()
    got = R.spatial_mean_bwd(d, 49, 8)
    _close(got[..., :5], x.grad, "spatial_mean_bwd")
    assert not got[..., 5:].any()


FOLD_PINS = [(6, 7, 0), (6, 7, 1), (9, 11, 4), (5, 6, 4), (5, 5, 4), (20, 27, 2), (4, 7, 3), (5, 6, 3), (2, 2, 1), (1, 1, 0)]


@pytest.mark.parametrize("geom", FOLD_PINS, ids=str)
def test_folds_are_the_adjoint_of_reflection_pad(geom):
    H, W, pad = geom
    B, C = 2, 3
    P = _rand(10, B, H + 2 * pad, W + 2 * pad, C)
    O = _rand(11, B, H, W, C)
    x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    F.pad(x, (pad, pad, pad, pad), mode="reflect").backward(P.permute(0, 3, 1, 2))
    adj = x.grad.permute(0, 2, 3, 1)
    _close(R.reflect_fold(P, H, W, pad), adj, "fold")
    _close(R.reflect_fold(P, H, W, pad, O, True), adj + O, "fold, accumulate")
    _close(R.reflect_fold_border(P, H, W, pad, O), O + adj - P[:, pad:pad + H, pad:pad + W], "border fold")
    s, a, n = R.reflect_fold(P, H, W, pad, O, True, terms=True)
    _close(a, R.reflect_fold(P.abs(), H, W, pad, O.abs(), True), "sum of |terms|")
    # at most three rows times three columns (where the bands overlap), plus the accumulated value
    assert n == max(len(_band_cells(h, H, pad)) for h in range(H)) * max(len(_band_cells(w, W, pad)) for w in range(W)) + 1 <= 10
    # the band form the kernels use gives the same sums, and names the cells the border fold touches
    _close(_fold_bands(P, H, W, pad), adj, "band form")
    touched = R.fold_touched(H, W, pad)
    same = R.reflect_fold_border(P, H, W, pad, O) == O
    assert bool(same[:, ~touched].all()) and int(touched.sum()) == _border_count(H, W, pad)


@pytest.mark.parametrize("case", K.CROP_CASES, ids=str)
def test_copy_crop_is_slicing_plus_zero_pad(case):
    (Hs, Ws), (Hd, Wd) = case
    src = _rand(12, 2, Hs, Ws, 5)
    h, w = min(Hs, Hd), min(Ws, Wd)
    want = F.pad(src[:, :h, :w], (0, 0, 0, Wd - w, 0, Hd - h))
    _close(R.copy_crop(src, Hd, Wd), want, "copy_crop")


def test_pack_grad_reads_the_strided_element_and_multiplies_in_f32():
    outer, inner, C = 2, 3, 5
    g = _rand(13, outer, C, inner).float()                              # (o, c, t): so = C * inner, st = 1, sc = inner
    y = torch.sigmoid(_rand(14, outer, C, inner)).float()
    mul = 0.75
    got = R.pack_grad(g, y, R.SIGMOID, outer, inner, C, C * inner, 1, inner, mul)
    want = (g * torch.tensor(mul)) * (y * (1.0 - y))
    assert got.dtype == torch.float32 and torch.equal(got, want.permute(0, 2, 1).reshape(outer * inner, C))
    g2 = _rand(15, outer, inner, 8).float()                             # rows wider than C
    got2 = R.pack_grad(g2, None, R.NONE, outer, inner, C, inner * 8, 8, 1)
    assert torch.equal(got2, g2[..., :C].reshape(outer * inner, C))


# ------------------------------------------------------------------------------------------------ wrong kernels
def _band_cells(i, n, pad, strict=False):
    """Padded cells of one axis that land on interior cell i, as the kernels enumerate them."""
    r = [i + pad]
    if 1 <= i and (i < pad if strict else i <= pad):
        r.append(pad - i)
    if n - 1 - pad <= i <= n - 2:
        r.append(2 * (n - 1) - i + pad)
    return r


def _fold_bands(P, H, W, pad, corners=True, strict=False, border_only=False):
    """The fold as the kernels index it: per interior cell the padded row h + pad plus the mirrored rows of the two bands
    1 <= h <= pad and H - 1 - pad <= h <= H - 2, the same for the columns, every combination summed.  corners=False leaves out
    the doubly mirrored cells; strict=True uses h < pad (w < pad) for the low band."""
    B, _, _, C = P.shape
    out = torch.zeros(B, H, W, C, dtype=torch.float64)
    for h in range(H):
        for w in range(W):
            for a, u in enumerate(_band_cells(h, H, pad, strict)):
                for c, v in enumerate(_band_cells(w, W, pad, strict)):
                    if (not corners and a and c) or (border_only and not a and not c):
                        continue
                    out[:, h, w] += P[:, u, v]
    return out


def _border_count(H, W, pad):
    """Pixels with a mirrored border cell: rows 1 .. pad and H - 1 - pad .. H - 2 (all columns) and the same columns elsewhere."""
    rows = {h for h in range(H) if 1 <= h <= pad or H - 1 - pad <= h <= H - 2}
    cols = {w for w in range(W) if 1 <= w <= pad or W - 1 - pad <= w <= W - 2}
    return len(rows) * W + (H - len(rows)) * len(cols)


def _bits_differ(wrong, want, mode):
    return not torch.equal(R.split(wrong, mode), R.split(want, mode))


def _beyond(wrong, want, tol):
    return bool(((wrong - want).abs() > tol).any())


def _one_clip(fn, x, *args):
    """`fn` with the clip boundary ignored: the frames of all clips as one sequence."""
    B, T = x.shape[:2]
    out = fn(x.reshape(1, B * T, *x.shape[2:]), *args)
    return out.reshape(B, T, *out.shape[2:])


def _stack_wrongs(x, kt, out_cs, mode):
    want = R.time_stack(x, kt, out_cs)
    C = x.shape[-1]
    pad = want.clone()
    pad[..., kt * C:] = x[..., :1]
    w = {"clip boundary ignored": _bits_differ(_one_clip(R.time_stack, x, kt, out_cs), want, mode),
         "padding channels left non-zero": _bits_differ(pad, want, mode)}
    if mode == "bf16x3":        # the thirds of the stack are the input's: without the low third the buffer holds hi | hi | 0
        b = R.split(want, mode)
        w["low third dropped"] = bool(b[..., 2 * out_cs:].any())
    return w


def _unstack_wrongs(d, C, kt, in_cs, mode):
    want = R.time_unstack(d, C, kt, in_cs)
    tol = R.sum_tol(want, R.time_unstack_abs(d, C, kt, in_cs), kt, mode)
    # t + dt - pt for t - dt + pt: the taps read in the opposite order
    flipped = R.time_unstack(d[..., :kt * C].reshape(*d.shape[:3], kt, C).flip(3).reshape(*d.shape[:3], kt * C), C, kt, in_cs)
    pad = want.clone()
    pad[..., C:] = d[..., :1]
    w = {"clip boundary ignored": _beyond(_one_clip(R.time_unstack, d, C, kt, in_cs), want, tol),
         "tap sign flipped": _beyond(flipped, want, tol),
         "padding channels left non-zero": _beyond(pad, want, tol)}
    if mode == "bf16x3":
        w["low third dropped"] = _beyond(R.store(want, "bf16"), want, tol)
    return w


def _seen(table, name):
    hits = [k for k, w in table.items() if w.get(name)]
    print(f"{name}: seen by {len(hits)} of {len(table)} (case, mode): {hits}")
    return bool(hits)


def test_the_time_stack_shapes_tell_a_wrong_kernel():
    table = {(case, mode): _stack_wrongs(K.stack_input(i, case, mode), case[5], case[6], mode)
             for i, case in enumerate(K.STACK_CASES) for mode in R.MODES}
    for name in ("clip boundary ignored", "padding channels left non-zero", "low third dropped"):
        assert _seen(table, name), name
    # the boundary shows wherever a clip has a neighbour and taps that leave it: every case but the copy
    for (case, mode), w in table.items():
        assert w["clip boundary ignored"] == (case[5] > 1), (case, mode)


def test_the_time_unstack_shapes_tell_a_wrong_kernel():
    table = {(case, mode): _unstack_wrongs(K.unstack_input(i, case, mode), case[3], case[5], case[4], mode)
             for i, case in enumerate(K.STACK_CASES) for mode in R.MODES}
    for name in ("clip boundary ignored", "tap sign flipped", "padding channels left non-zero", "low third dropped"):
        assert _seen(table, name), name


def test_the_spatial_mean_shapes_tell_a_wrong_kernel():
    fwd, bwd = {}, {}
    for i, case in enumerate(K.MEAN_CASES):
        N, HW, C, cs, modes = case
        for mode in modes:
            x = K.mean_input(i, case, mode)
            want = R.spatial_mean(x)
            tol = R.sum_tol(want, x.abs().sum(1), HW, mode, divisor=HW)
            w = {"mean over HW - 1 pixels": _beyond(x[:, :-1].sum(1) / HW, want, tol),
                 "mean divided by HW + 1": _beyond(x.sum(1) / (HW + 1), want, tol)}
            if mode == "bf16x3":
                w["low third dropped"] = _beyond(R.store(want, "bf16"), want, tol)
            fwd[(case[:4], mode)] = w
            d = K.mean_bwd_input(i, case, mode)
            wb = R.spatial_mean_bwd(d, HW, cs)
            tb = R.sum_tol(wb, R.spatial_mean_bwd(d.abs(), HW, cs), 1, mode)
            pad = wb.clone()
            pad[..., C:] = (d[:, :1] / HW)[:, None, :]
            b = {"mean divided by HW + 1": _beyond(wb * HW / (HW + 1), wb, tb),
                 "padding channels left non-zero": cs > C and _beyond(pad, wb, tb)}
            if mode == "bf16x3":
                b["low third dropped"] = _beyond(R.store(wb, "bf16"), wb, tb)
            bwd[(case[:4], mode)] = b
    for name in ("mean over HW - 1 pixels", "mean divided by HW + 1", "low third dropped"):
        assert _seen(fwd, name), name
    for name in ("mean divided by HW + 1", "padding channels left non-zero", "low third dropped"):
        assert _seen(bwd, name), name
    # one pixel of 49 (and of 196 in the three-pass mode) is far outside the bound
    assert fwd[((6, 49, 24, 32), "bf16")]["mean over HW - 1 pixels"]
    assert fwd[((3, 196, 8, 16), "bf16x3")]["mean over HW - 1 pixels"]


NO_CORNERS, STRICT_BAND = "fold without the doubly mirrored corner terms", "fold band h < pad instead of h <= pad"


def test_the_fold_shapes_tell_a_wrong_kernel():
    table = {}
    for i, (H, W, pad, C, _, _) in enumerate(K.FOLD_CASES):
        for mode in R.MODES:
            P, O = K.fold_inputs(i, H, W, pad, C, mode)
            for acc in (False, True):
                want, a, n = R.reflect_fold(P, H, W, pad, O, acc, terms=True)
                tol = R.sum_tol(want, a, n, mode)
                base = O if acc else 0.0
                w = {NO_CORNERS: _beyond(_fold_bands(P, H, W, pad, corners=False) + base, want, tol),
                     STRICT_BAND: _beyond(_fold_bands(P, H, W, pad, strict=True) + base, want, tol)}
                if mode == "bf16x3":
                    w["low third dropped"] = _beyond(R.store(want, "bf16"), want, tol)
                table[((H, W, pad, C), mode, acc)] = w
    for name in (NO_CORNERS, STRICT_BAND, "low third dropped"):
        assert _seen(table, name), name
    # both show at every pad >= 1, in every mode
    for (geom, mode, acc), w in table.items():
        assert w[STRICT_BAND] == (geom[2] >= 1) and w[NO_CORNERS] == (geom[2] >= 1)
    border = {}
    for i, (H, W, pad, C) in enumerate(K.BORDER_GEOMS):
        for mode in R.MODES:
            P, O = K.fold_inputs(40 + i, H, W, pad, C, mode, B=K.BORDER_B)
            want, a, n = R.reflect_fold_border(P, H, W, pad, O, terms=True)
            tol = R.sum_tol(want, a, n, mode)
            border[((H, W, pad, C), mode)] = {
                NO_CORNERS: _beyond(_fold_bands(P, H, W, pad, corners=False, border_only=True) + O, want, tol),
                STRICT_BAND: _beyond(_fold_bands(P, H, W, pad, strict=True, border_only=True) + O, want, tol)}
    for name in (NO_CORNERS, STRICT_BAND):
        assert all(w[name] for w in border.values()), name


def _crop_source_pitch(src, Hd, Wd):
    """copy_crop that indexes the DESTINATION pixel with the source's row pitch Ws (writes past the buffer dropped)."""
    B, Hs, Ws, C = src.shape
    out = torch.zeros(B * Hd * Wd, C, dtype=torch.float64)
    for b in range(B):
        for h in range(Hd):
            for w in range(Wd):
                i = (b * Hd + h) * Ws + w
                if i < out.shape[0]:
                    out[i] = src[b, h, w] if h < Hs and w < Ws else 0.0
    return out.reshape(B, Hd, Wd, C)


def test_the_crop_shapes_tell_a_wrong_kernel():
    table = {}
    for i, case in enumerate(K.CROP_CASES):
        (Hs, Ws), (Hd, Wd) = case
        for mode in R.MODES:
            src = K.crop_input(i, case, 64, mode)
            want = R.copy_crop(src, Hd, Wd)
            w = {"crop indexing the destination with the source pitch": _bits_differ(_crop_source_pitch(src, Hd, Wd), want, mode)}
            if mode == "bf16x3":
                w["low third dropped"] = bool(R.split(want, mode)[..., 128:].any())
            table[(case, mode)] = w
            assert w["crop indexing the destination with the source pitch"] == (Ws != Wd), case
    for name in ("crop indexing the destination with the source pitch", "low third dropped"):
        assert _seen(table, name), name
