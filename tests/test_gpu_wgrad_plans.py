"""Every route, kernel instance and plan of the weight-gradient kernels (csrc/wgrad.hip) against the float64 reference of
tests/wgrad_reference.py, in the three storage modes.

Tiled route: every plan the library offers for a shape (wgrad_pin.Pinner.offered: the full product of plan values, kept where
sos_wgrad_tune_load accepts the line) is PINNED through the plan table, verified through sos_wgrad_describe to be what the descriptor
resolves to, and launched.  The other routes (split-K GEMM, thin 1x1, thin taps) have no plan: their shapes, splits and knobs are
launched as they resolve.  tests/test_wgrad_plans_host_cpu.py shows on the CPU that this list reaches every kernel instance and every
feature of a launch.

EXACT inputs: operands k/4, |k| <= 4 (bf16x3: lo thirds j 2^-8, |j| <= 4, written into the segments directly), power-of-two scales.
Every product is a multiple of one power of two and the reference asserts sum |g||x| below 2^24 of them, so every partial sum in
every order, split and plan is an f32 value and dw must EQUAL the reference bit for bit: a dropped border k-step, a wrong tap offset,
a stale or missing partial plane is an exact mismatch.  The operands are dense NHWC with non-zero g_off / x_off, cs > off + M and NaN
in every channel outside the owned range (a row of dW depends on its own channel only); the workspace and (accumulate = 0) dw are
prefilled with NaN; guard elements around dw must not change.

ROUNDING: realistic values at the default plan of every shape and route, elementwise |dw - ref| <= n 2^-24 sum |g||x| with n = non-zero
terms + partial planes + 5: the classical bound of any summation order under round-to-nearest additions, taken against the reference
(the products of two 16-bit operands are exact in f32).  bf16x3 runs three launches: their planes are added up in n."""
import atexit
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_pin as P
import wgrad_reference as R
from util import hashed

pytestmark = pytest.mark.gpu
if P.forcing_switch():
    pytest.skip(P.forcing_switch(), allow_module_level=True)

GUARD = 1024                # sentinel floats before and behind dw (and behind an exactly sized workspace)
SENTINEL = -7.25
DEV = "cuda"
_PINNERS, _OPERANDS, _STATS = {}, {}, {}


@pytest.fixture(params=["bf16", "bf16x3", "fp16"])
def mode(request):
    import sos_amd
    sos_amd.set_precision(request.param)
    try:
        yield request.param
    finally:
        sos_amd.set_precision("bf16")


def pinner_of(mode):
    which = "fp16" if mode == "fp16" else "bf16"
    if which not in _PINNERS:
        _PINNERS[which] = P.Pinner()
        atexit.register(_PINNERS[which].close)    # (the scratch table file)
        P.assert_not_shipped(_PINNERS[which], P.TILED_SHAPES)
    return _PINNERS[which]


def _storage(mode):
    return torch.float16 if mode == "fp16" else torch.bfloat16


def _round(v, mode):
    return torch.from_numpy(v).to(torch.float32).to(_storage(mode)).to(torch.float64).numpy()


def _values(idx, shape, mode, kind, lo=False):
    """float64 values the 16-bit buffer will hold exactly."""
    if kind == "exact":
        return R.grid_values(idx, shape, step=2.0 ** -8 if lo else 0.25)
    v = hashed(idx, shape).astype(np.float64)
    hi = _round(v, mode)
    return _round(v - hi, mode) if lo else hi


class Operands:
    """The two operands of a shape on the device and the reference of their gradient (computed once, never changed).  16-bit modes:
    [B][H][W][cs] with the owned channels at [OFF, OFF + M); bf16x3: hi|hi|lo thirds of cs channels each, the owned channels at
    OFF inside every third.  Every other channel holds NaN."""

    def __init__(self, s, mode, kind):
        self.s, self.x3 = s, mode == "bf16x3"
        g_cs, g_off, x_cs, x_off = P.layout(s)
        self.cs = (g_cs, x_cs)
        Hx, Wx = s.x_hw
        nseg = 3 if self.x3 else 1
        g = np.full((s.B, s.Hg, s.Wg, nseg * g_cs), np.nan)
        x = np.full((s.B, Hx, Wx, nseg * x_cs), np.nan)
        for arr, cs, off, n, (h, w), idx in ((g, g_cs, g_off, s.M, (s.Hg, s.Wg), 1), (x, x_cs, x_off, s.n_x, (Hx, Wx), 2)):
            hi = _values(10 * idx, (s.B, h, w, n), mode, kind)
            arr[..., off:off + n] = hi
            if self.x3:
                arr[..., cs + off:cs + off + n] = hi
                arr[..., 2 * cs + off:2 * cs + off + n] = _values(10 * idx + 1, (s.B, h, w, n), mode, kind, lo=True)
        kw = dict(g_off=g_off, M=s.M, x_off=x_off, N=s.N, kh=s.k[0], kw=s.k[1], stride=s.stride, dil=s.dil, pad=s.padding,
                  pad_mode=R.REFLECT if s.reflect else R.ZERO,
                  temporal=None if not s.temporal else (s.temporal[0], s.temporal[1], (s.temporal[1] - 1) // 2, s.temporal[2]))
        self.ref, self.sabs, self.nterms = R.reference_x3(g, x, g_cs, x_cs, **kw) if self.x3 else R.reference(g, x, **kw)
        if kind == "exact":
            own = lambda a, cs, off, n, t: a[..., t * cs + off:t * cs + off + n]
            pairs = [(own(g, g_cs, g_off, s.M, gt), own(x, x_cs, x_off, s.n_x, xt)) for gt, xt in (R.X3_PASSES if self.x3 else ((0, 0),))]
            self.q = R.assert_exact(pairs, None, self.sabs)
        self._np, self._dev = (g, x), {}
        self.dw0 = R.grid_values(7, self.ref.shape)                     # the preset gradient of the accumulating launches

    def on_device(self, mode):
        """(g, x) in the storage type of `mode` (the exact 16-bit operands hold the same values in bf16 and fp16)"""
        dt = _storage(mode)
        if dt not in self._dev:
            self._dev[dt] = tuple(torch.from_numpy(a).to(dt).to(DEV).contiguous() for a in self._np)
        return self._dev[dt]


def operands(s, mode, kind):
    key = (s.name, "16" if kind == "exact" and mode != "bf16x3" else mode, kind)
    if key not in _OPERANDS:
        _OPERANDS[key] = Operands(s, mode, kind)
    return _OPERANDS[key]


def _f32(ref):
    t = torch.from_numpy(ref).to(torch.float32)
    assert bool((t.to(torch.float64) == torch.from_numpy(ref)).all()), "the expected gradient is not an f32 value"
    return t.to(DEV)


class Rig:
    """One shape's descriptor on device buffers (16-bit modes)."""

    def __init__(self, s, ops, h, mode):
        from sos_amd import _lib as L
        self.s, self.ops, self.h, self.L = s, ops, h, L
        self.d = d = P.geometry_desc(s)
        self.g, self.x = ops.on_device(mode)
        d.g, d.x = self.g.data_ptr(), self.x.data_ptr()
        need = h.sos_wgrad_workspace_bytes(C.byref(d))
        assert need > 0
        self.ws = torch.empty(need // 4, dtype=torch.float32, device=DEV)
        self.plane = s.k[0] * s.k[1] * ((s.M + 31) // 32 * 32) * ((s.N + 31) // 32 * 32)
        self.n = s.M * s.N * s.k[0] * s.k[1]
        self.buf = torch.empty(2 * GUARD + self.n, dtype=torch.float32, device=DEV)
        self.dw0 = _f32(ops.dw0).reshape(-1)
        self.scale_dev = torch.tensor([2.0 ** -3], dtype=torch.float32, device=DEV)
        self.launches = 0

    def run(self, accumulate=False, scaled=False, ksplit=0, halves=False):
        """Launch and return dw (device, f32 [M][N][kh][kw]); asserts the guards.  ksplit > 0: a workspace of exactly
        sos_wgrad_workspace_bytes with a guard behind it."""
        d, h, L = self.d, self.h, self.L
        d.ksplit = ksplit
        if ksplit > 0:
            need = h.sos_wgrad_workspace_bytes(C.byref(d))
            assert need == ksplit * self.plane * 4
            ws = torch.full((need // 4 + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
            ws[need // 4:] = SENTINEL
        else:
            rc, info = P.describe(h, d)
            assert rc == 0
            ws = self.ws
            ws[:info.ksplit * self.plane] = float("nan")
        self.buf.fill_(SENTINEL)
        self.buf[GUARD:GUARD + self.n] = self.dw0 if accumulate else float("nan")
        d.partial, d.dw = ws.data_ptr(), self.buf.data_ptr() + 4 * GUARD
        d.accumulate, d.scale, d.scale_dev = int(accumulate), (0.5 if scaled else 1.0), (self.scale_dev.data_ptr() if scaled else None)
        if halves:
            L.check(h.sos_conv2d_wgrad_partial(C.byref(d), L.stream_ptr()), "sos_conv2d_wgrad_partial")
            L.check(h.sos_conv2d_wgrad_reduce(C.byref(d), L.stream_ptr()), "sos_conv2d_wgrad_reduce")
        else:
            L.check(h.sos_conv2d_wgrad(C.byref(d), L.stream_ptr()), "sos_conv2d_wgrad")
        self.launches += 1
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all()), "a guard around dw changed"
        if ksplit > 0:
            assert bool((ws[-GUARD:] == SENTINEL).all()), "the guard behind the workspace changed"
        d.ksplit = 0
        return self.buf[GUARD:GUARD + self.n].clone()

    def expected(self, accumulate=False, scaled=False):
        sc = 2.0 ** -4 if scaled else 1.0
        R.assert_exact([(np.array([2.0 ** -self.ops.q]), np.array([1.0]))], None, self.ops.sabs, scale=sc,
                       dw0=self.ops.dw0 if accumulate else None)
        return _f32((self.ops.dw0 if accumulate else 0.0) + sc * self.ops.ref).reshape(-1)

    def check_exact(self, tag, **kw):
        halves = kw.pop("halves", False)
        got = self.run(halves=halves, **{k: v for k, v in kw.items()})
        want = self.expected(kw.get("accumulate", False), kw.get("scaled", False))
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got)
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{self.s.name} {tag} {kw}: {int(bad.sum())} of {self.n} elements differ, first at {i}: "
                                 f"{float(got[i])} != {float(want[i])}")
        return got

    def variants(self, tag):
        """accumulate, scale x scale_dev, explicit splits, the two halves."""
        fused = self.check_exact(tag)
        self.check_exact(tag, accumulate=True)
        self.check_exact(tag, scaled=True)
        self.check_exact(tag, accumulate=True, scaled=True)
        for ksplit in (1, 2, 7):
            self.check_exact(tag, ksplit=ksplit)
        assert torch.equal(self.check_exact(tag, halves=True), fused)
        self.check_exact(tag, halves=True, accumulate=True, scaled=True, ksplit=2)


def _count(mode, n):
    st = _STATS.setdefault(mode, dict(launches=0, share=0.0))
    st["launches"] += n
    print(f"wgrad plans {mode}: {n} launches, so far {st}")


def _acts(ops, s):
    """engine.Act views of the bf16x3 operands."""
    from sos_amd import engine as E
    Hx, Wx = s.x_hw
    ga = E.Act(s.B, s.Hg, s.Wg, ops.cs[0], True, torch.device(DEV))
    xa = E.Act(s.B, Hx, Wx, ops.cs[1], True, torch.device(DEV))
    ga.t, xa.t = ops.on_device("bf16x3")
    return ga, xa


def _engine_wgrad(ops, s, accumulate=False, scale=1.0):
    """One engine.wgrad (three launches in bf16x3) into a NaN-prefilled, guarded dw."""
    from sos_amd import engine as E, _lib as L
    ga, xa = _acts(ops, s)
    n = s.M * s.N * s.k[0] * s.k[1]
    buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.float32, device=DEV)
    dw = buf[GUARD:GUARD + n].view(s.M, s.N, s.k[0], s.k[1])
    dw.copy_(_f32(ops.dw0)) if accumulate else dw.fill_(float("nan"))
    E.wgrad(ga, P.OFF, s.M, xa, P.OFF, s.N, s.k[0], s.k[1], dw, stride=s.stride, dil=s.dil, pad=s.padding,
            pad_mode=L.PAD_REFLECT if s.reflect else L.PAD_ZERO, accumulate=accumulate, scale=scale,
            temporal=None if not s.temporal else s.temporal)
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "a guard around dw changed"
    return dw.reshape(-1).clone()


def _x3_exact(ops, s, tag):
    got = _engine_wgrad(ops, s)
    want = _f32(ops.ref).reshape(-1)
    assert torch.equal(got, want), f"{s.name} bf16x3 {tag}: {int(((got != want) | torch.isnan(got)).sum())} elements differ"
    R.assert_exact([(np.array([2.0 ** -ops.q]), np.array([1.0]))], None, ops.sabs, scale=0.5, dw0=ops.dw0)
    got = _engine_wgrad(ops, s, accumulate=True, scale=0.5)
    assert torch.equal(got, _f32(ops.dw0 + 0.5 * ops.ref).reshape(-1)), f"{s.name} bf16x3 {tag}: accumulate, scale"


@pytest.mark.parametrize("s", P.TILED_SHAPES, ids=[s.name for s in P.TILED_SHAPES])
def test_every_offered_plan_is_bit_exact(s, mode, monkeypatch):
    pn = pinner_of(mode)
    ops = operands(s, mode, "exact")
    geom = P.geometry_desc(s)
    plans = pn.offered(geom)
    assert plans and pn.default_plan(geom) in plans
    if mode == "bf16x3":                          # through engine.wgrad: the default plan and three others spread over the list
        picks = [pn.default_plan(geom)] + [plans[i * (len(plans) - 1) // 2] for i in range(3)]
        for plan in picks:
            pn.pin(geom, plan)
            _x3_exact(ops, s, plan)
        _count(mode, 6 * len(picks))
        return
    rig = Rig(s, ops, pn.h, mode)
    infos = [(plan, pn.pin(rig.d, plan)) for plan in plans]
    extra = P.variants(infos)
    for plan, _ in infos:
        pn.pin(rig.d, plan)
        if plan in extra:
            rig.variants(plan)
        else:
            rig.check_exact(plan)
    if s.k == (5, 5) and s.M >= 64:               # the plain twins of the balanced 25-tap instances
        monkeypatch.setenv("SOS_WGRAD_NOBAL", "1")
        for plan, info in infos:
            if info.v == 1 and plan in extra:
                assert pn.pin(rig.d, plan).instance == ("wgrad", info.mt, 1, 0)
                rig.check_exact((plan, "plain twin"))
    _count(mode, rig.launches)


@pytest.mark.parametrize("s", P.GEMM_SHAPES, ids=[s.name for s in P.GEMM_SHAPES])
def test_gemm_route_is_bit_exact(s, mode, monkeypatch):
    pn = pinner_of(mode)
    ops = operands(s, mode, "exact")
    if mode == "bf16x3":
        for split in (None, 2):
            if split:
                monkeypatch.setenv("SOS_WGG_SPLIT", str(split))
            _x3_exact(ops, s, f"split {split}")
        return _count(mode, 12)
    rig = Rig(s, ops, pn.h, mode)
    assert P.describe(pn.h, rig.d)[1].instance == ("gemm", 0, 0, 0)
    rig.variants("automatic split")
    for split in (1, 2, 3):
        monkeypatch.setenv("SOS_WGG_SPLIT", str(split))
        info = P.describe(pn.h, rig.d)[1]
        assert info.route == "gemm" and info.ksplit == split
        rig.check_exact(f"split {split}")
        rig.check_exact(f"split {split}", accumulate=True, scaled=True)
    _count(mode, rig.launches)


THIN_GROUPS = [(m, n) for m, n in P.THIN_MN]


@pytest.mark.parametrize("mn", THIN_GROUPS, ids=["%dx%d" % mn for mn in THIN_GROUPS])
def test_thin_route_is_bit_exact(mn, mode, monkeypatch):
    pn = pinner_of(mode)
    for s in (s for s in P.THIN_SHAPES if (s.M, s.N) == mn):
        ops = operands(s, mode, "exact")
        if mode == "bf16x3":
            _x3_exact(ops, s, "thin")
            _count(mode, 6)
            continue
        rig = Rig(s, ops, pn.h, mode)
        info = P.describe(pn.h, rig.d)[1]
        assert info.route == "thin" and info.instance == ("thin", (s.M + 15) // 16, (s.N + 15) // 16, 0)
        rig.variants("thin")
        monkeypatch.setenv("SOS_WGT_OCC", "2")
        assert P.describe(pn.h, rig.d)[1].route == "thin"
        rig.check_exact("two workgroups per CU")
        rig.check_exact("two workgroups per CU", accumulate=True, scaled=True)
        monkeypatch.delenv("SOS_WGT_OCC")
        _count(mode, rig.launches)


@pytest.mark.parametrize("s", P.TAPS_SHAPES, ids=[s.name for s in P.TAPS_SHAPES])
def test_thin_taps_route_is_bit_exact(s, mode):
    pn = pinner_of(mode)
    ops = operands(s, mode, "exact")
    if mode == "bf16x3":
        _x3_exact(ops, s, "thin taps")
        return _count(mode, 6)
    rig = Rig(s, ops, pn.h, mode)
    assert P.describe(pn.h, rig.d)[1].instance == ("thin_taps", 4, 5, 0)
    rig.variants("thin taps")
    _count(mode, rig.launches)


ROUNDING_SHAPES = P.ALL_SHAPES


@pytest.mark.parametrize("s", ROUNDING_SHAPES, ids=[s.name for s in ROUNDING_SHAPES])
def test_rounding_error_stays_within_the_summation_bound(s, mode):
    """Realistic values, the default plan: |dw - ref| <= n 2^-24 sum |g||x| elementwise, n = non-zero terms + partial planes + 5."""
    pn = pinner_of(mode)
    ops = operands(s, mode, "hashed")
    geom = P.geometry_desc(s)
    rc, info = P.describe(pn.h, geom)
    assert rc == 0
    if info.route == "tiled":
        info = pn.pin(geom, pn.default_plan(geom))
    if mode == "bf16x3":
        got, planes = _engine_wgrad(ops, s), 3 * info.ksplit
    else:
        rig = Rig(s, ops, pn.h, mode)
        got, planes = rig.run(), info.ksplit
    got = got.double().cpu().numpy().reshape(ops.ref.shape)
    assert not np.isnan(got).any()
    bound = (ops.nterms + planes + 5) * 2.0 ** -24 * ops.sabs
    err = np.abs(got - ops.ref)
    share = float(np.max(err / np.maximum(bound, 1e-300)))
    st = _STATS.setdefault(mode, dict(launches=0, share=0.0))
    st["share"] = max(st["share"], share)
    print(f"wgrad rounding {mode} {s.name}: route {info.route} {info.instance} ksplit {info.ksplit}: worst share of the bound {share:.4f}"
          f" (max err {err.max():.3e}, max |ref| {np.abs(ops.ref).max():.3e}); so far {st}")
    assert (err <= bound).all(), f"{s.name}: worst share of the bound {share}"
