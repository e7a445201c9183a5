"""The small kernels that move activations and gradients between the big ones, each at its own entry point against the float64
references of tests/glue_reference.py, in the three storage modes (bf16, fp16, bf16x3):

  csrc/video.hip : sos_time_stack, sos_time_unstack, sos_spatial_mean, sos_spatial_mean_bwd
  csrc/bn.hip    : sos_copy_crop, sos_reflect_fold, sos_reflect_fold_border, sos_pack_grad_f32

Inputs are tests/glue_cases.py's (hashed, O(1), already stored once in the mode under test, so every term is exact).  Every
output buffer is filled with a NaN bit pattern before the call and everything outside the documented written region is compared
bit for bit afterwards.  Tolerances are derived, not measured:
  relocations (time_stack, copy_crop, pack_grad): the stored bit patterns must be split(value) exactly, zero is bit zero;
  sums (time_unstack <= kt terms, folds <= 9 (+ 1) terms, mean HW terms / HW, mean_bwd 1 term / HW): glue_reference.sum_tol --
  one store of a sum of n exact terms accumulated in f32; in the three-pass mode the first two thirds are bit-identical and the
  low third is the stored rest.
tests/test_glue_reference.py shows on the CPU that a kernel wrong in any of the listed ways misses these bounds at these shapes.
Each test prints `glue-slack`: the largest error as a fraction of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import glue_cases as K
import glue_reference as R
from test_gpu_train_ops import _act_from_nchw, _act_to_nchw, mode_x3        # noqa: F401  (mode_x3 is a fixture)
from util import hashed

pytestmark = pytest.mark.gpu

SENT = 0x7FC1               # a NaN in bfloat16 and in IEEE half
EINVAL = -22                # SOS_EINVAL of include/sos_hip.h


def _L():
    from sos_amd import _lib as L
    return L


def _mode():
    import sos_amd
    return sos_amd.get_precision()


def _report(kernel, mode, frac):
    print(f"glue-slack kernel={kernel} mode={mode} frac={frac:.3f}")


class Buf:
    """A 16-bit device buffer [npix, nseg * row] (thirds hi | hi | lo, `row` apart, in bf16x3), every element the sentinel."""

    def __init__(self, npix, row, mode):
        self.npix, self.row, self.mode = npix, row, mode
        self.nseg = 3 if mode == "bf16x3" else 1
        self.bits = torch.full((npix, self.nseg * row), SENT, dtype=torch.int16, device="cuda")

    def put(self, c_off, v):
        """Store float64 [npix, C] at channels [c_off, c_off + C) of every third."""
        v = v.reshape(self.npix, -1)
        C = v.shape[1]
        b = R.split(v, self.mode).cuda()
        for s in range(self.nseg):
            self.bits[:, s * self.row + c_off:s * self.row + c_off + C] = b[:, s * C:(s + 1) * C]

    def get(self, c_off, C):
        """int16 [npix, nseg * C] on the CPU: the thirds of the channels [c_off, c_off + C) side by side (split()'s layout)."""
        return torch.cat([self.bits[:, s * self.row + c_off:s * self.row + c_off + C] for s in range(self.nseg)], dim=1).cpu()

    def view(self, c_off, C):
        v = _L().View()
        v.ptr, v.npix, v.row, v.c_off, v.C = self.bits.data_ptr(), self.npix, self.nseg * self.row, c_off, C
        v.x3, v.third = (1 if self.nseg == 3 else 0), self.row
        return v

    @property
    def ptr(self):
        return ctypes.c_void_p(self.bits.data_ptr())

    def assert_rest(self, before, c_off, C, pix=None, what=""):
        """Everything but the channels [c_off, c_off + C) of every third (of the pixels `pix`: bool [npix]) is bit-identical."""
        written = torch.zeros_like(self.bits, dtype=torch.bool)
        for s in range(self.nseg):
            written[:, s * self.row + c_off:s * self.row + c_off + C] = True
        if pix is not None:
            written &= pix.to(written.device)[:, None]
        assert torch.equal(self.bits[~written], before[~written]), f"{what}: wrote outside its region"


def _call(name, *args):
    L = _L()
    rc = getattr(L.lib(), name)(*args, L.stream_ptr())
    L.check(rc, name)
    torch.cuda.synchronize()


def _assert_bits(got, want, what):
    bad = got != want
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} stored patterns differ, "
                                 f"first at {bad.nonzero()[0].tolist()}")


def _assert_sum(kernel, buf, c_off, want, abs_terms, n, divisor=1.0):
    """The channels [c_off, c_off + C) of `buf` hold `want` [npix, C] (float64) within the bound of a stored f32 sum."""
    mode = buf.mode
    want, abs_terms = want.reshape(buf.npix, -1).cpu(), abs_terms.reshape(buf.npix, -1).cpu()
    C = want.shape[1]
    b = buf.get(c_off, C)
    got = R.held(b, mode)
    tol = R.sum_tol(want, abs_terms, n, mode, divisor)
    err = (got - want).abs()
    frac = float((err / tol.clamp_min(1e-300)).max())
    _report(kernel, mode, frac)
    assert bool((err <= tol).all()), f"{kernel} {mode}: error {frac:.3f} of the bound at {(err > tol).nonzero()[0].tolist()}"
    if mode == "bf16x3":
        assert torch.equal(b[:, :C], b[:, C:2 * C]), f"{kernel}: the first two thirds differ"
        hi, lo = b[:, :C].view(torch.bfloat16).double(), b[:, 2 * C:].view(torch.bfloat16).double()
        rest, acc = want - hi, R.f32_term(abs_terms, n, divisor)
        assert bool((rest.abs() <= 2.0 ** -8 * want.abs() + acc).all()), f"{kernel}: hi is not the rounded sum"
        assert bool(((lo - rest).abs() <= 2.0 ** -8 * (rest.abs() + acc) + acc).all()), f"{kernel}: lo is not the stored rest"


# ------------------------------------------------------------------------------------------------ video glue
@pytest.mark.parametrize("i", range(len(K.STACK_CASES)), ids=[str(c) for c in K.STACK_CASES])
def test_time_stack(i, mode_x3):
    case = K.STACK_CASES[i]
    B, T, HW, C, in_cs, kt, out_cs = case
    mode = _mode()
    x = K.stack_input(i, case, mode)
    src, dst = Buf(B * T * HW, in_cs, mode), Buf(B * T * HW, out_cs, mode)      # (the padding channels of src stay NaN: never read)
    src.put(0, x)
    _call("sos_time_stack", src.ptr, B, T, HW, C, in_cs, src.nseg, kt, dst.ptr, out_cs)
    want = R.split(R.time_stack(x, kt, out_cs).reshape(-1, out_cs), mode)
    _assert_bits(dst.get(0, out_cs), want, f"time_stack {case}")


@pytest.mark.parametrize("i", range(len(K.STACK_CASES)), ids=[str(c) for c in K.STACK_CASES])
def test_time_unstack(i, mode_x3):
    case = K.STACK_CASES[i]
    B, T, HW, C, in_cs, kt, st_cs = case
    mode = _mode()
    d = K.unstack_input(i, case, mode)                      # non-zero in the padding channels too: the kernel must not add them
    src, dst = Buf(B * T * HW, st_cs, mode), Buf(B * T * HW, in_cs, mode)
    src.put(0, d)
    _call("sos_time_unstack", src.ptr, B, T, HW, C, st_cs, src.nseg, kt, dst.ptr, in_cs)
    _assert_sum("time_unstack", dst, 0, R.time_unstack(d, C, kt, in_cs), R.time_unstack_abs(d, C, kt, in_cs), kt)
    assert not bool(dst.get(C, in_cs - C).any()), "padding channels of the frame gradient are not bit zero"


MEAN_RUNS = [(i, m) for i, c in enumerate(K.MEAN_CASES) for m in c[4]]


@pytest.fixture(params=MEAN_RUNS, ids=[f"{K.MEAN_CASES[i][:4]}-{m}" for i, m in MEAN_RUNS])
def mean_run(request):
    import sos_amd
    i, mode = request.param
    sos_amd.set_precision(mode)
    try:
        yield i, K.MEAN_CASES[i], mode
    finally:
        sos_amd.set_precision("bf16")


def test_spatial_mean(mean_run):
    i, (N, HW, C, in_cs, _), mode = mean_run
    x = K.mean_input(i, K.MEAN_CASES[i], mode)
    src, feat = Buf(N * HW, in_cs, mode), Buf(N, K.FEAT_ROW, mode)
    src.put(0, x)
    before = feat.bits.clone()
    _call("sos_spatial_mean", src.ptr, N, HW, C, in_cs, src.nseg, feat.ptr, feat.nseg * K.FEAT_ROW, K.FEAT_ROW, K.FEAT_OFF)
    _assert_sum("spatial_mean", feat, K.FEAT_OFF, R.spatial_mean(x), x.abs().sum(1), HW, divisor=HW)
    feat.assert_rest(before, K.FEAT_OFF, C, what="spatial_mean")


def test_spatial_mean_bwd(mean_run):
    i, (N, HW, C, cs, _), mode = mean_run
    d = K.mean_bwd_input(i, K.MEAN_CASES[i], mode)
    feat, dy = Buf(N, K.FEAT_ROW, mode), Buf(N * HW, cs, mode)
    feat.put(K.FEAT_OFF, d)
    _call("sos_spatial_mean_bwd", feat.ptr, N, HW, C, feat.nseg * K.FEAT_ROW, K.FEAT_ROW, K.FEAT_OFF, feat.nseg, dy.ptr, cs)
    _assert_sum("spatial_mean_bwd", dy, 0, R.spatial_mean_bwd(d, HW, cs), R.spatial_mean_bwd(d.abs(), HW, cs) * HW, 1, divisor=HW)
    assert not bool(dy.get(C, cs - C).any()), "padding channels of the activation gradient are not bit zero"


# ------------------------------------------------------------------------------------------------ crop
def _crop(sv, Hs, Ws, dv, Hd, Wd):
    _call("sos_copy_crop", ctypes.byref(sv), Hs, Ws, ctypes.byref(dv), Hd, Wd)


@pytest.mark.parametrize("i", range(len(K.CROP_CASES)), ids=[str(c) for c in K.CROP_CASES])
def test_copy_crop(i, mode_x3):
    """64 channels read at c_off = 64 of a 128-wide source, written at c_off = 64 of a 192-wide destination whose neighbouring
    64-channel parts (live data of a concat buffer) must come back bit-identical."""
    case = K.CROP_CASES[i]
    (Hs, Ws), (Hd, Wd) = case
    mode, B = _mode(), K.CROP_B
    x = K.crop_input(i, case, 64, mode)
    src, dst = Buf(B * Hs * Ws, 128, mode), Buf(B * Hd * Wd, 192, mode)
    src.put(0, K.values(190, (B * Hs * Ws, 64), mode))
    src.put(64, x)
    dst.put(0, K.values(191, (B * Hd * Wd, 64), mode))
    dst.put(128, K.values(192, (B * Hd * Wd, 64), mode))
    before = dst.bits.clone()
    _crop(src.view(64, 64), Hs, Ws, dst.view(64, 64), Hd, Wd)
    _assert_bits(dst.get(64, 64), R.split(R.copy_crop(x, Hd, Wd).reshape(-1, 64), mode), f"copy_crop {case}")
    dst.assert_rest(before, 64, 64, what="copy_crop")


@pytest.mark.parametrize("i", [0, 1], ids=[str(c) for c in K.CROP_CASES[:2]])
def test_copy_crop_of_12_channels_moves_the_run_rounded_up_to_8(i, mode_x3):
    """The contract of include/sos_hip.h: a view's C is rounded up to whole 8-channel runs.  C = 12 at c_off = 8: the destination
    channels [8, 20) are the crop, [20, 24) are the crop of the SOURCE's channels [12, 16) (the caller owns them), and nothing at
    or beyond c_off + 16 -- nor below c_off -- changes."""
    case = K.CROP_CASES[i]
    (Hs, Ws), (Hd, Wd) = case
    mode, B = _mode(), K.CROP_B
    x = K.crop_input(i, case, 16, mode)                     # 12 channels and the 4 that share their second run
    src, dst = Buf(B * Hs * Ws, 16, mode), Buf(B * Hd * Wd, 32, mode)
    src.put(0, x)
    dst.put(0, K.values(193, (B * Hd * Wd, 32), mode))
    before = dst.bits.clone()
    _crop(src.view(0, 12), Hs, Ws, dst.view(8, 12), Hd, Wd)
    want = R.split(R.copy_crop(x, Hd, Wd).reshape(-1, 16), mode)
    _assert_bits(dst.get(8, 16), want, f"copy_crop C=12 {case}")
    dst.assert_rest(before, 8, 16, what="copy_crop C=12")


# ------------------------------------------------------------------------------------------------ folds
def _fold(pv, H, W, pad, ov, accumulate):
    _call("sos_reflect_fold", ctypes.byref(pv), H, W, pad, ctypes.byref(ov), 1 if accumulate else 0)


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("i", range(len(K.FOLD_CASES)), ids=[str(c) for c in K.FOLD_CASES])
def test_reflect_fold(i, accumulate, mode_x3):
    H, W, pad, C, c_off, row = K.FOLD_CASES[i]
    mode, B = _mode(), K.FOLD_B
    P, O = K.fold_inputs(i, H, W, pad, C, mode)
    pb, ob = Buf(B * (H + 2 * pad) * (W + 2 * pad), (C + 15) // 16 * 16, mode), Buf(B * H * W, row, mode)
    pb.put(0, P)
    if accumulate:                                          # (store: the slice holds NaN patterns, which a read would spread)
        ob.put(c_off, O)
    before = ob.bits.clone()
    _fold(pb.view(0, C), H, W, pad, ob.view(c_off, C), accumulate)
    want, a, n = R.reflect_fold(P, H, W, pad, O, accumulate, terms=True)
    _assert_sum("reflect_fold", ob, c_off, want, a, n)
    ob.assert_rest(before, c_off, C, what="reflect_fold")


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_reflect_fold_of_12_channels_moves_the_run_rounded_up_to_8(accumulate, mode_x3):
    """C = 12 at c_off = 8 of a 32-wide gradient: [8, 20) is the fold; [20, 24) is the fold of the PADDED tensor's channels
    [12, 16) (added to what was there when accumulating): the caller owns that padding; [0, 8) and [24, 32) do not change."""
    H, W, pad = 6, 7, 1
    mode, B = _mode(), K.FOLD_B
    P, O = K.fold_inputs(30, H, W, pad, 16, mode)
    pb, ob = Buf(B * (H + 2 * pad) * (W + 2 * pad), 16, mode), Buf(B * H * W, 32, mode)
    pb.put(0, P)
    ob.put(0, K.values(231, (B * H * W, 32), mode))
    ob.put(8, O)
    before = ob.bits.clone()
    _fold(pb.view(0, 12), H, W, pad, ob.view(8, 12), accumulate)
    want, a, n = R.reflect_fold(P, H, W, pad, O, accumulate, terms=True)
    _assert_sum("reflect_fold C=12", ob, 8, want, a, n)
    ob.assert_rest(before, 8, 16, what="reflect_fold C=12")


def test_reflect_fold_as_the_plain_add_of_two_channels(mode_x3):
    """denoiser/networks.py adds the loss gradient on n_pred (2 channels of a 16-wide pack whose other channels are ZERO) onto
    the 16-wide gradient buffer with pad = 0, C = 2, accumulate.  Channels [0, 2) are the sum; [2, 8) share the run: zero is
    added, so they keep their VALUE (re-stored: bit-identical in the 16-bit modes); [8, 16) are not touched."""
    H, W, mode, B = 6, 7, _mode(), K.FOLD_B
    P = K.values(240, (B, H, W, 2), mode)
    O = K.values(241, (B * H * W, 16), mode)
    pb, ob = Buf(B * H * W, 16, mode), Buf(B * H * W, 16, mode)
    pb.put(0, torch.zeros(B * H * W, 16, dtype=torch.float64))
    pb.put(0, P)
    ob.put(0, O)
    before = ob.bits.clone()
    _fold(pb.view(0, 2), H, W, 0, ob.view(0, 2), True)
    want, a, n = R.reflect_fold(P, H, W, 0, O[:, :2].reshape(B, H, W, 2), True, terms=True)
    assert n == 2
    _assert_sum("reflect_fold C=2", ob, 0, want, a, n)
    assert torch.equal(R.held(ob.get(2, 6), mode), O[:, 2:8]), "the channels that share the run changed value"
    if mode != "bf16x3":
        ob.assert_rest(before, 0, 2, what="reflect_fold C=2")
    ob.assert_rest(before, 0, 8, what="reflect_fold C=2")


@pytest.mark.parametrize("i", range(len(K.BORDER_GEOMS)), ids=["%dx%d pad%d c%d" % g for g in K.BORDER_GEOMS])
def test_reflect_fold_border(i, mode_x3):
    """The geometries of test_gpu_train_ops.test_reflect_fold_border_adds_the_mirrored_cells (the border kernel, bands that meet,
    pad = H - 2, the all-pixel fallback at pad = H - 1) in every mode with the derived bound; cells without a mirrored border
    cell keep their bits."""
    from sos_amd import train_ops as TO
    H, W, pad, C = K.BORDER_GEOMS[i]
    mode = _mode()
    P, O = K.fold_inputs(40 + i, H, W, pad, C, mode, B=K.BORDER_B)
    pa, pheld = _act_from_nchw(P.permute(0, 3, 1, 2).float(), mode_x3)
    oa, oheld = _act_from_nchw(O.permute(0, 3, 1, 2).float(), mode_x3)
    assert torch.equal(pheld.double(), P.permute(0, 3, 1, 2)) and torch.equal(oheld.double(), O.permute(0, 3, 1, 2))
    before = oa.t.clone()
    TO.reflect_fold_border(pa, H, W, pad, oa, 0, C)
    torch.cuda.synchronize()
    want, a, n = R.reflect_fold_border(P, H, W, pad, O, terms=True)
    got = _act_to_nchw(oa, C).permute(0, 2, 3, 1).double()
    tol = R.sum_tol(want, a, n, mode)
    err = (got - want).abs()
    tol = tol.clamp_min(1e-300)
    _report("reflect_fold_border", mode, float((err / tol).max()))
    assert bool((err <= tol).all()), (K.BORDER_GEOMS[i], mode, float((err / tol).max()))
    touched = R.fold_touched(H, W, pad)
    assert torch.equal(oa.t[:, ~touched].view(torch.int16), before[:, ~touched].view(torch.int16)), "interior pixel rewritten"
    assert torch.equal(oa.t.view(oa.B, H, W, oa.nseg, oa.cs)[..., C:].view(torch.int16),
                       before.view(oa.B, H, W, oa.nseg, oa.cs)[..., C:].view(torch.int16)), "channels beyond C changed"


# ------------------------------------------------------------------------------------------------ f32 gradient pack
def pack_grad_path(act, C, so, st, sc, total, c_off, row):
    """Mirror of sos_pack_grad_f32's choice: the 8-channels-per-thread row kernel for channel-contiguous, 16-byte aligned
    sources without the sigmoid derivative, else the element kernel."""
    rows = (sc == 1 and act != R.SIGMOID and C % 8 == 0 and total // 8 < 0x7fffffff and so % 4 == 0 and st % 4 == 0
            and c_off % 8 == 0 and row % 8 == 0)
    return "rows" if rows else "element"


PACK_CASES = [("rows", 1600, 37 * 1600, "rows"), ("C=1596", 1596, 37 * 1600, "element"),
              ("so%4", 1600, 37 * 1600 + 2, "element")]


@pytest.mark.parametrize("case", PACK_CASES, ids=[c[0] for c in PACK_CASES])
def test_pack_grad_rows_with_mul_into_a_wider_destination(case, mode_x3):
    """Channel-contiguous gradients times a non-unit `mul` into c_off = 16 of a wider destination: the row kernel, and the
    element kernel for C % 8 != 0 and for so % 4 != 0.  Exact: one store of the f32 product."""
    _, C, so, path = case
    L, mode = _L(), _mode()
    B, T, st, row = 3, 37, 1600, 1632
    assert pack_grad_path(R.NONE, C, so, st, 1, B * T * C, 16, row) == path
    g = torch.from_numpy(hashed(81, (B * so,)).astype(np.float32)).cuda()
    mul = torch.tensor([0.7], dtype=torch.float32, device="cuda")
    dst = Buf(B * T, row, mode)
    before = dst.bits.clone()
    v = dst.view(16, C)
    _call("sos_pack_grad_f32", L.ptr(g), None, L.ACT_NONE, B, T, C, so, st, 1, ctypes.byref(v), L.ptr(mul))
    want = R.pack_grad(g.cpu(), None, R.NONE, B, T, C, so, st, 1, float(mul))
    _assert_bits(dst.get(16, C), R.split(want, mode), f"pack_grad {case[0]}")
    dst.assert_rest(before, 16, C, what="pack_grad")


def test_pack_grad_strided_sigmoid(mode_x3):
    """The mask head's form (channel stride T, times y (1 - y) of the f32 output) with `mul`, into c_off = 8 of a 64-wide
    destination (three thirds in bf16x3): exact after one store of the f32 product."""
    L, mode = _L(), _mode()
    B, T, C = 3, 37, 48
    assert pack_grad_path(R.SIGMOID, C, C * T, 1, T, B * T * C, 8, 64) == "element"
    g = torch.from_numpy(hashed(82, (B, C, T)).astype(np.float32)).cuda()
    y = torch.sigmoid(torch.from_numpy(hashed(83, (B, C, T)).astype(np.float32))).cuda()
    mul = torch.tensor([0.7], dtype=torch.float32, device="cuda")
    dst = Buf(B * T, 64, mode)
    before = dst.bits.clone()
    v = dst.view(8, C)
    _call("sos_pack_grad_f32", L.ptr(g), L.ptr(y), L.ACT_SIGMOID, B, T, C, C * T, 1, T, ctypes.byref(v), L.ptr(mul))
    want = R.pack_grad(g.cpu(), y.cpu(), R.SIGMOID, B, T, C, C * T, 1, T, float(mul))
    _assert_bits(dst.get(8, C), R.split(want, mode), "pack_grad sigmoid'")
    dst.assert_rest(before, 8, C, what="pack_grad sigmoid'")


# ------------------------------------------------------------------------------------------------ second grid-stride trip
GRID_CAP_BN = 768 * 256             # grid_for of bn.hip: at most 768 workgroups of 256 threads
GRID_CAP_VIDEO = 65536 * 256        # the launchers of video.hip


@pytest.fixture(params=["bf16", "fp16"])
def mode16(request):
    import sos_amd
    sos_amd.set_precision(request.param)
    try:
        yield request.param
    finally:
        sos_amd.set_precision("bf16")


def _big(idx, shape, mode):
    """Device float64 `shape` of stored hashed values: a block of 1000003 of them repeated (no period of any geometry here)."""
    n = int(np.prod(shape))
    base = K.values(idx, (1000003,), mode).cuda()
    return base.repeat(n // base.numel() + 1)[:n].reshape(shape)


def _dev_buf(v, mode):
    """Device int16 rows of float64 values that are already stored ones (16-bit modes)."""
    return v.reshape(-1, v.shape[-1]).to(torch.float16 if mode == "fp16" else torch.bfloat16).view(torch.int16).contiguous()


def _raw_view(bits, c_off, C):
    v = _L().View()
    v.ptr, v.npix, v.row, v.c_off, v.C, v.x3, v.third = bits.data_ptr(), bits.shape[0], bits.shape[1], c_off, C, 0, 0
    return v


def _held16(bits, mode):
    return bits.view(torch.float16 if mode == "fp16" else torch.bfloat16).double()


def test_copy_crop_beyond_one_grid(mode16):
    B, (Hs, Ws), (Hd, Wd), C = 2, (66, 199), (64, 200), 64
    assert B * Hd * Wd * C // 8 > GRID_CAP_BN
    x = _big(300, (B, Hs, Ws, C), mode16)
    src = _dev_buf(x, mode16)
    dst = torch.full((B * Hd * Wd, C), SENT, dtype=torch.int16, device="cuda")
    sv, dv = _raw_view(src, 0, C), _raw_view(dst, 0, C)
    _crop(sv, Hs, Ws, dv, Hd, Wd)
    assert torch.equal(_held16(dst, mode16), R.copy_crop(x, Hd, Wd).reshape(-1, C)) and not bool((dst == SENT).any())


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_reflect_fold_beyond_one_grid(accumulate, mode16):
    B, H, W, pad, C = 2, 64, 200, 2, 64
    assert B * H * W * C // 8 > GRID_CAP_BN
    P, O = _big(301, (B, H + 2 * pad, W + 2 * pad, C), mode16), _big(302, (B, H, W, C), mode16)
    pb = _dev_buf(P, mode16)
    ob = _dev_buf(O, mode16) if accumulate else torch.full((B * H * W, C), SENT, dtype=torch.int16, device="cuda")
    pv, ov = _raw_view(pb, 0, C), _raw_view(ob, 0, C)
    _fold(pv, H, W, pad, ov, accumulate)
    want, a, n = R.reflect_fold(P, H, W, pad, O, accumulate, terms=True)
    err, tol = (_held16(ob, mode16).reshape(want.shape) - want).abs(), R.sum_tol(want, a, n, mode16)
    _report("reflect_fold(big)", mode16, float((err / tol).max()))
    assert bool((err <= tol).all())


def test_time_unstack_beyond_one_grid(mode16):
    B, T, HW, C, kt = 2, 4, 33000, 64, 3
    assert B * T * HW * C > GRID_CAP_VIDEO
    d = _big(303, (B, T, HW, kt * C), mode16)
    src = _dev_buf(d, mode16)
    dst = torch.full((B * T * HW, C), SENT, dtype=torch.int16, device="cuda")
    _call("sos_time_unstack", ctypes.c_void_p(src.data_ptr()), B, T, HW, C, kt * C, 1, kt, ctypes.c_void_p(dst.data_ptr()), C)
    want, a = R.time_unstack(d, C, kt, C), R.time_unstack_abs(d, C, kt, C)
    err, tol = (_held16(dst, mode16).reshape(want.shape) - want).abs(), R.sum_tol(want, a, kt, mode16)
    _report("time_unstack(big)", mode16, float((err / tol).max()))
    assert bool((err <= tol).all())


def test_spatial_mean_bwd_beyond_one_grid(mode16):
    N, HW, C = 8, 33000, 64
    assert N * HW * C > GRID_CAP_VIDEO
    d = K.values(304, (N, C), mode16).cuda()
    feat = _dev_buf(d, mode16)
    dy = torch.full((N * HW, C), SENT, dtype=torch.int16, device="cuda")
    _call("sos_spatial_mean_bwd", ctypes.c_void_p(feat.data_ptr()), N, HW, C, C, C, 0, 1, ctypes.c_void_p(dy.data_ptr()), C)
    want = R.spatial_mean_bwd(d, HW, C)
    err, tol = (_held16(dy, mode16).reshape(want.shape) - want).abs(), R.sum_tol(want, want.abs() * HW, 1, mode16, divisor=HW)
    _report("spatial_mean_bwd(big)", mode16, float((err / tol).max()))
    assert bool((err <= tol).all())


def test_time_stack_beyond_one_grid(mode16):
    """270 MB of output: the relocation is checked on the bit patterns themselves (exact as float64 integers)."""
    B, T, HW, C, kt = 2, 4, 88000, 64, 3
    assert B * T * HW * kt * C // 8 > GRID_CAP_VIDEO
    src = _dev_buf(_big(305, (B, T, HW, C), mode16), mode16)
    dst = torch.full((B * T * HW, kt * C), SENT, dtype=torch.int16, device="cuda")
    _call("sos_time_stack", ctypes.c_void_p(src.data_ptr()), B, T, HW, C, C, 1, kt, ctypes.c_void_p(dst.data_ptr()), kt * C)
    want = R.time_stack(src.reshape(B, T, HW, C), kt, kt * C).to(torch.int16)
    assert torch.equal(dst.reshape(want.shape), want)


# ------------------------------------------------------------------------------------------------ host-side rejections
def test_bad_arguments_are_refused_before_any_launch():
    """Every call returns SOS_EINVAL from the host-side checks; the buffers are real and large enough for the nearest valid
    geometry, and no argument is one an entry point accepts."""
    L = _L()
    lib, s = L.lib(), L.stream_ptr()
    a, b = Buf(2 * 5 * 6, 16, "bf16"), Buf(2 * 5 * 6, 16, "bf16")
    before = (a.bits.clone(), b.bits.clone())
    bad = {
        "stack: even kt": lib.sos_time_stack(a.ptr, 2, 5, 6, 3, 16, 1, 4, b.ptr, 16, s),
        "stack: out_cs % 8": lib.sos_time_stack(a.ptr, 2, 5, 6, 3, 16, 1, 3, b.ptr, 12, s),
        "stack: out_cs < kt C": lib.sos_time_stack(a.ptr, 2, 5, 6, 3, 16, 1, 5, b.ptr, 8, s),
        "stack: C > in_cs": lib.sos_time_stack(a.ptr, 2, 5, 6, 3, 2, 1, 3, b.ptr, 16, s),
        "stack: nseg 2": lib.sos_time_stack(a.ptr, 2, 5, 6, 3, 16, 2, 3, b.ptr, 16, s),
        "unstack: even kt": lib.sos_time_unstack(a.ptr, 2, 5, 6, 3, 16, 1, 2, b.ptr, 16, s),
        "unstack: st_cs < kt C": lib.sos_time_unstack(a.ptr, 2, 5, 6, 3, 8, 1, 3, b.ptr, 16, s),
        "unstack: C > in_cs": lib.sos_time_unstack(a.ptr, 2, 5, 6, 3, 16, 1, 3, b.ptr, 2, s),
        "unstack: nseg 2": lib.sos_time_unstack(a.ptr, 2, 5, 6, 3, 16, 2, 3, b.ptr, 16, s),
        "mean: C > in_cs": lib.sos_spatial_mean(a.ptr, 10, 6, 3, 2, 1, b.ptr, 16, 16, 0, s),
        "mean: nseg 2": lib.sos_spatial_mean(a.ptr, 10, 6, 3, 16, 2, b.ptr, 16, 16, 0, s),
        "mean_bwd: C > cs": lib.sos_spatial_mean_bwd(a.ptr, 10, 6, 3, 16, 16, 0, 1, b.ptr, 2, s),
        "mean_bwd: nseg 2": lib.sos_spatial_mean_bwd(a.ptr, 10, 6, 3, 16, 16, 0, 2, b.ptr, 16, s),
    }
    # folds: padded 2 x (3 + 2 pad)^2 pixels would be needed; pad >= H is refused whatever the buffers hold
    pv, ov = a.view(0, 16), b.view(0, 16)
    ov.npix = 2 * 3 * 3
    for pad in (3, 4):
        pv.npix = 2 * (3 + 2 * pad) * (3 + 2 * pad)
        bad[f"fold: pad {pad} >= H"] = lib.sos_reflect_fold(ctypes.byref(pv), 3, 3, pad, ctypes.byref(ov), 0, s)
        bad[f"fold border: pad {pad} >= H"] = lib.sos_reflect_fold_border(ctypes.byref(pv), 3, 3, pad, ctypes.byref(ov), s)
    # crop: 2 source images, 3 destination images
    sv, dv = a.view(0, 16), b.view(0, 16)
    sv.npix, dv.npix = 2 * 2 * 5, 3 * 2 * 5
    bad["crop: image counts differ"] = lib.sos_copy_crop(ctypes.byref(sv), 2, 5, ctypes.byref(dv), 2, 5, s)
    assert all(rc == EINVAL for rc in bad.values()), {k: rc for k, rc in bad.items() if rc != EINVAL}
    torch.cuda.synchronize()
    assert torch.equal(a.bits, before[0]) and torch.equal(b.bits, before[1])
