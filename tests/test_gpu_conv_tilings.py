"""Every kernel instance and tile geometry of the forward convolution (csrc/conv.hip) against the float64 reference of
tests/conv_reference.py, in the three storage modes.

Each tiling is PINNED for its shape through the tiling table (tests/conv_pin.py: one-line table, sos_conv2d_tune_load, the
descriptor must resolve to the table's entry) and launched on EXACT inputs: integers and dyadic fractions for which every partial
sum in every order is an f32 value (the reference asserts it), so the f32 output must equal the reference and the 16-bit output its
round-to-nearest-even, bit for bit, for every tiling: a dropped, doubled or misplaced tap, channel chunk, residue class or pixel is
an exact mismatch.  The output buffer lies inside a larger allocation filled with a NaN pattern -- before it, behind it, in the
channels around [out_c_off, out_c_off + cout_store) and in the columns a ragged batch leaves alone -- and the WHOLE allocation is
compared bitwise: a store of an overhanging tile is a mismatch too.

The bounds of this file are the two derived ones: Sigmoid (1 storage ulp at the reference + F32_EVAL of tests/test_gpu_batchnorm.py)
and the random-valued case ((n_terms + 2) 2^-24 sum |w||x|, + 1 storage ulp for 16-bit outputs).

What runs per shape is capped by conv_pin.select(): every ks code offered x one tiling of every geometry kind offered."""
import atexit
import ctypes as C

import numpy as np
import pytest
import torch

import conv_pin as P
import conv_reference as R

pytestmark = pytest.mark.gpu
if P.forcing_switch():
    pytest.skip(P.forcing_switch(), allow_module_level=True)
P.assert_not_shipped([P.geometry_desc(s, m, o) for s in P.ALL_SHAPES for m in ("bf16", "bf16x3") for o in ("16", "f32", "f32s")])

GUARD = 4096                # sentinel elements before and behind the output buffer
TAIL = 8                    # at least this many sentinel channels behind [out_c_off, out_c_off + cout_store)
_PINNERS = {}
DEV = "cuda"


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
    return _PINNERS[which]


def _dev(t, dtype):
    return t.to(dtype).to(DEV).contiguous()


class Rig:
    """One descriptor on device buffers + the expected content of the whole output allocation."""

    def __init__(self, s, mode, out="16", act=R.PRELU, epilogue="exact", gen=(R.exact_input, R.exact_weight), in_extra=0, cin_off=0,
                 c_off=0, store_extra=0, round8=False, accumulate=False, stats=False, ragged=None, gather=False, in_bn=False,
                 exact=True, seed=0):
        from sos_amd import _lib as L
        self.L, self.s, self.mode, self.out, self.exact = L, s, mode, out, exact
        x3 = mode == "bf16x3"
        st = R.storage_dtype(mode)
        nseg = 3 if x3 else 1
        Wp = (s.W + 1) // 2 if gather else s.W                 # nearest resize x2: logical column j reads physical column j / 2
        x = gen[0](300 + seed, (s.B, s.H, Wp, s.cin), mode)
        w = gen[1](400 + seed, (s.cout, s.cin, s.k[0], s.k[1]), mode)
        cs_in = s.cin + in_extra
        cstore = s.cout + store_extra
        if round8:
            cstore = (cstore + 7) // 8 * 8
        scale = shift = None
        if epilogue == "exact":
            scale, shift = R.exact_epilogue(s.cout_pad)
        elif epilogue == "stats":
            scale, shift = R.stats_epilogue(s.cout_pad)
        c = R.Case(inp=R.pack_input(x, cs_in, mode, cin_off, fill=3.0 if in_extra else None), wgt=R.pack_weight(w, s.cin, mode),
                   cin=s.cin, cout=s.cout, kh=s.k[0], kw=s.k[1], Ho=s.Ho, Wo=s.Wo, cin_off=cin_off, in_nseg=nseg, in_seg_stride=cs_in,
                   stride=s.stride, dil_h=s.dil[0], dil_w=s.dil[1], pad_top=s.pad[0], pad_left=s.pad[1],
                   pad_mode=R.REFLECT if s.reflect else R.ZERO, cout_store=cstore, scale=scale, shift=shift, act=act, slope=0.25,
                   stats_c=s.cout if stats else 0, wl_tab=ragged, wo_tab=ragged)
        if gather:
            c.w_gather = torch.arange(s.W) // 2
        if in_bn:
            ch = torch.arange(s.cin)
            c.in_scale, c.in_shift = 2.0 ** -(ch % 2).double(), ((ch % 3).double() - 1) / 64 + 1
        Ct = (c_off + cstore + 7) // 8 * 8 + TAIL      # (rows of whole 16-byte pieces, as every engine buffer)
        row = (nseg if out == "16" else 1) * Ct
        shape = (s.B, Ct, s.Ho, s.Wo) if out == "f32s" else (s.B, s.Ho, s.Wo, row)
        odt = st if out == "16" else torch.float32
        n = s.B * s.Ho * s.Wo * row
        init = torch.full((GUARD + n + GUARD,), float("nan"), dtype=odt)
        body = init[GUARD:GUARD + n].view(shape)
        if accumulate:
            c.prev = R._hash_int(500 + seed, (s.B, s.Ho, s.Wo, cstore), -64, 64).double() / 2 + (2.0 ** -9 if x3 else 0.0)
            ph, pl = R.split_storage(c.prev, mode)
            assert torch.equal(ph + (pl if x3 else 0), c.prev)
            self._write(body, ph, pl if x3 else None, c_off, Ct, [s.Wo] * s.B)
        self.c = c
        self.r = R.reference(c, mode, exact=exact)
        exp = init.clone()
        ebody = exp[GUARD:GUARD + n].view(shape)
        cols = ragged if ragged is not None else [s.Wo] * s.B
        if out == "16":
            hi, lo = R.stored(c, self.r, mode, exact=exact)
            self._write(ebody, hi, lo, c_off, Ct, cols)
        else:
            y = R.stored(c, self.r, mode, out="f32")
            for b in range(s.B):
                if out == "f32s":
                    ebody[b, c_off:c_off + cstore, :, :cols[b]] = y[b, :, :cols[b]].permute(2, 0, 1)
                else:
                    ebody[b, :, :cols[b], c_off:c_off + cstore] = y[b, :, :cols[b]]
        self.shape, self.n, self.c_off, self.cstore, self.Ct = shape, n, c_off, cstore, Ct
        self.bits = torch.int16 if out == "16" else torch.int32
        self.init_dev, self.exp_dev = init.to(DEV), exp.to(DEV)
        self.out_dev = torch.empty_like(self.init_dev)
        self.keep = [_dev(c.inp, st), _dev(c.wgt, st)]
        d = P.geometry_desc(s, mode, out, gather=gather)
        d.W, d.Wl = Wp, s.W
        d.in_, d.wgt = self.keep[0].data_ptr(), self.keep[1].data_ptr()
        d.in_cs, d.cin_off, d.in_seg_stride = nseg * cs_in, cin_off, cs_in
        d.out = self.out_dev.data_ptr() + GUARD * self.out_dev.element_size()
        d.out_c_off, d.cout_store, d.out_third = c_off, cstore, Ct
        if out == "f32s":
            d.out_sc, d.out_sw, d.out_sh, d.out_sb = s.Ho * s.Wo, 1, s.Wo, Ct * s.Ho * s.Wo
        else:
            d.out_sc, d.out_sw, d.out_sh, d.out_sb = 1, row, s.Wo * row, s.Ho * s.Wo * row
        if scale is not None:
            self.keep += [_dev(scale, torch.float32), _dev(shift, torch.float32)]
            d.scale, d.shift = self.keep[-2].data_ptr(), self.keep[-1].data_ptr()
        d.act = act
        if act == R.PRELU:
            self.keep.append(torch.tensor([c.slope], dtype=torch.float32, device=DEV))
            d.act_param = self.keep[-1].data_ptr()
        d.accumulate = 1 if accumulate else 0
        if ragged is not None:
            self.keep += [torch.tensor(ragged, dtype=torch.int32, device=DEV)] * 2
            d.wl_tab, d.wo_tab = self.keep[-1].data_ptr(), self.keep[-1].data_ptr()
        if gather:
            self.keep.append(_dev(c.w_gather, torch.int32))
            d.w_gather = self.keep[-1].data_ptr()
        if in_bn:
            self.keep += [_dev(c.in_scale, torch.float32), _dev(c.in_shift, torch.float32)]
            d.in_scale, d.in_shift = self.keep[-2].data_ptr(), self.keep[-1].data_ptr()
        self.stats = stats
        if stats:
            d.stats_c = s.cout
            self.ref_stats = R.statistics(c, self.r, mode, exact=exact)
        self.d = d
        self.pinner = pinner_of(mode)

    def _write(self, body, hi, lo, c_off, Ct, cols):
        cs = hi.shape[-1]
        for b in range(hi.shape[0]):
            v = hi[b, :, :cols[b]].to(body.dtype)
            body[b, :, :cols[b], c_off:c_off + cs] = v
            if self.mode == "bf16x3":
                body[b, :, :cols[b], Ct + c_off:Ct + c_off + cs] = v
                body[b, :, :cols[b], 2 * Ct + c_off:2 * Ct + c_off + cs] = lo[b, :, :cols[b]].to(body.dtype)

    def tilings(self):
        return P.select(P.offered(self.pinner, self.d))

    def launch(self, t):
        """Pin the tiling, launch on a pristine output allocation; returns the statistics partials summed over the tiles."""
        NC, TH, TW, ks = t[:4]
        tiles = self.pinner.pin(self.d, NC, TH, TW, ks)
        self.out_dev.copy_(self.init_dev)
        part = None
        if self.stats:
            part = torch.full((2, self.d.stats_c, tiles), float("nan"), dtype=torch.float32, device=DEV)
            self.d.stats = part.data_ptr()
        self.L.check(self.L.lib().sos_conv2d_fwd(C.byref(self.d), self.L.stream_ptr()), f"sos_conv2d_fwd {self.s.name} {t}")
        return part

    def body(self, t=None):
        return (self.out_dev if t is None else t)[GUARD:GUARD + self.n].view(self.shape)

    def check_exact(self, t):
        part = self.launch(t)
        got, want = self.out_dev.view(self.bits), self.exp_dev.view(self.bits)
        if not torch.equal(got, want):
            bad = got != want
            inside = int(bad[GUARD:GUARD + self.n].sum())
            first = int(bad.nonzero()[0]) - GUARD
            idx = [int(i) for i in np.unravel_index(first, self.shape)] if 0 <= first < self.n else first
            raise AssertionError(f"{self.s.name} {self.mode} out={self.out} tiling {t} -> instance {P.decode(t[3], self.d)}: "
                                 f"{int(bad.sum())} elements differ ({inside} inside the buffer, the rest in the guards), first at "
                                 f"{idx}: got {self.out_dev[first + GUARD].item()} want {self.exp_dev[first + GUARD].item()}")
        if part is not None:
            got_st = part.double().sum(dim=2).cpu()
            assert torch.equal(got_st, self.ref_stats), (f"{self.s.name} {self.mode} tiling {t}: fused statistics differ in "
                                                         f"{int((got_st != self.ref_stats).sum())} of {got_st.numel()} sums")

    def run_all(self, tilings=None, check=None):
        tilings = self.tilings() if tilings is None else tilings
        assert tilings, f"{self.s.name}: no tiling to run"
        for t in tilings:
            (check or self.check_exact)(t)
        torch.cuda.synchronize()
        return len(tilings)


def _report(what, s, mode, n, rig):
    inst = len({P.decode(t[3], rig.d) for t in rig.tilings()})
    print(f"[conv-tilings] {what} {s.name} {mode}: {n} (instance, geometry) pairs, {inst} instances")


# ------------------------------------------------------------------------------------------------ a. every instance, plain descriptor
@pytest.mark.parametrize("s", P.PLAIN_SHAPES, ids=lambda s: s.name)
def test_every_instance_and_geometry_plain_descriptor(s, mode):
    """f32 output and dense 16-bit output of every (ks code, geometry kind) offered for the shape.  The epilogue rotates over the
    kernel's three staged branches (raw accumulators, fma + ReLU, fma + PReLU); the three-per-CU and 384-slot instances store
    whole 8-channel pieces, so they run with cout_store rounded up to 8 (zero filled), everything else with cout_store = cout
    (partial pieces where cout % 8 != 0)."""
    i = P.PLAIN_SHAPES.index(s)
    act, epi = [(R.NONE, None), (R.RELU, "exact"), (R.PRELU, "exact")][i % 3]
    n = 0
    for out in ("f32", "16"):
        rig = Rig(s, mode, out, act=act, epilogue=epi, seed=i)
        special = [t for t in rig.tilings() if not P.runs_as_pinned(rig.d, t[3])]
        n += rig.run_all([t for t in rig.tilings() if t not in special])
        if special:
            rig8 = Rig(s, mode, out, act=act, epilogue=epi, seed=i, round8=True)
            assert all(P.runs_as_pinned(rig8.d, t[3]) for t in special)
            n += rig8.run_all(special)
    _report("plain", s, mode, n, rig)


# ------------------------------------------------------------------------------------------------ b. stride 2
@pytest.mark.parametrize("s", P.STRIDE2_SHAPES, ids=lambda s: s.name)
def test_stride_two_reflect(s, mode):
    """DownConvBlock geometry (5x5 taps, stride 2, reflection padding, odd H and W): every ks code x every tile kind offered."""
    n = 0
    for out in ("f32", "16"):
        rig = Rig(s, mode, out, seed=40)
        assert len({t[3] for t in rig.tilings()}) >= 2 and len(rig.tilings()) >= 2 * len({t[3] for t in rig.tilings()}) - 1
        n += rig.run_all()
    _report("stride 2", s, mode, n, rig)


# ------------------------------------------------------------------------------------------------ c. descriptor features x tilings
def _kinds_present(rig, tilings, mode):
    kinds = {t[4] for t in tilings}
    assert "pow2" in kinds and kinds & {"npot", "npot-odd", "classes-npot", "classes3"}, kinds
    if rig.s.dil[1] > 1:
        assert kinds & {"classes", "classes3", "classes-npot"}, kinds


FEATURES = {
    "cin_off": dict(in_extra=32, cin_off=16),
    "c_off+zero-fill": dict(c_off=8, store_extra=8),
    "accumulate": dict(accumulate=True, c_off=8),
    "statistics": dict(stats=True, gen=(R.stats_input, R.stats_weight), epilogue="stats", act=R.RELU),
    "ragged": dict(ragged="ragged"),
    "gather": dict(gather=True),
    "f32-strided": dict(out="f32s"),
}


@pytest.mark.parametrize("feature", sorted(FEATURES))
@pytest.mark.parametrize("s", P.FEATURE_SHAPES, ids=lambda s: s.name)
def test_descriptor_features_under_every_tiling_kind(s, feature, mode):
    """Each descriptor feature under a power-of-two tile, a non-power-of-two tile, a multi-class tile (where the shape is dilated)
    and -- where plan() allows it -- the three-per-CU and 384-slot instances.  Where plan() refuses the instance for the
    descriptor (three per CU with accumulation or a hi|hi|lo / partial-piece output, 384 slots with a ragged batch), pin() must
    fail: with the reason for three per CU (its plain twin would run), with the cost model's candidate listed for 384 slots."""
    kw = dict(FEATURES[feature])
    if kw.get("ragged"):
        kw["ragged"] = [s.Wo, 5]                  # clip 1 is narrower than every tile but the 1-wide ones
    rig = Rig(s, mode, seed=50, **kw)
    tilings = rig.tilings()
    _kinds_present(rig, tilings, mode)
    runs = [t for t in tilings if P.runs_as_pinned(rig.d, t[3])]
    refused = [t for t in tilings if t not in runs]
    n = rig.run_all(runs)
    for t in refused:
        with pytest.raises(AssertionError, match="plain twin|cfg 0/"):
            rig.pinner.pin(rig.d, *t[:4])
    codes = {t[3] // 100 for t in tilings if t[3] > 0 and t[3] < 1000}
    if mode != "bf16x3" and feature not in ("f32-strided",):
        assert {2, 3} <= codes, f"{s.name}: no three-per-CU / 384-slot tiling offered ({sorted(codes)})"
        if feature in ("cin_off", "statistics", "gather", "c_off+zero-fill"):
            assert not refused, refused           # dense16 holds: these instances really ran the feature
        if feature == "accumulate":
            assert {t[3] // 100 for t in refused} == {2}
        if feature == "ragged":
            assert {t[3] // 100 for t in refused} == {3}
    print(f"[conv-tilings] {feature} {s.name} {mode}: {n} pairs ran, {len(refused)} refused by plan() as expected")


@pytest.mark.parametrize("s", P.FEATURE_SHAPES, ids=lambda s: s.name)
def test_fused_input_batchnorm(s, mode):
    """sos_conv_desc.in_scale on the two instances built for it (three n-tiles, two slab buffers, 2 and 3 k-steps): the input is
    max(x * in_scale + in_shift, 0) rounded to storage while it is staged, zero padding stays zero.  Other k-step counts and
    bf16x3 are refused with the reason."""
    if mode == "bf16x3":
        rig = Rig(s, "bf16x3", seed=60)
        rig.d.in_scale = rig.d.in_shift = rig.keep[0].data_ptr()
        assert rig.pinner.resolved(rig.d)[0] < 0 and "fused input BatchNorm" in rig.pinner.h.sos_last_error().decode()
        return
    rig = Rig(s, mode, seed=60, in_bn=True)
    tilings = [t for t in rig.tilings() if P.decode(t[3], rig.d) in ((False, 3, 2, 2, False, 256), (False, 3, 3, 2, False, 256))]
    assert {t[3] for t in tilings} == ({2, 3} if s.cin == 96 else {3})

    def staged(t):
        """plan(): the fused staging moves at most 64 instructions of 64 / (2 ks + 1) patch pixels"""
        NC, TH, TW, ks = t[:4]
        ppi = 64 // (2 * ks + 1)
        return -(-NC * (TH - 1 + s.k[0]) * (TW - 1 + s.k[1]) // ppi) <= 64
    runs = [t for t in tilings if staged(t)]
    _kinds_present(rig, runs, mode)
    n = rig.run_all(runs)
    # every other tiling is refused for this descriptor -- larger patches (1 x 256 and 128 x 2 tiles: before plan() knew the limit
    # they ran on a patch whose end was never staged), other k-step counts, single slab: the cost model's candidate runs instead
    refused = [t for t in tilings if t not in runs] + [t for t in rig.tilings() if t not in tilings][:3]
    assert len(refused) > 3 or s.cin != 96
    for t in refused:
        assert rig.pinner.load(P.shape_key(rig.d), *t[:4]) == 1
        tiles, listed = rig.pinner.resolved(rig.d)
        assert "cfg 0/" in listed and tiles > 0, f"{t}: taken from the table for a descriptor with in_scale"
    print(f"[conv-tilings] fused input BatchNorm {s.name} {mode}: {n} pairs, {len(refused)} refused by plan() as expected")


def test_sigmoid_epilogue(mode):
    """The one inexact epilogue: exact accumulators, y = 1 / (1 + expf(-z)) in f32.
    16-bit outputs: within 1 storage ulp at the reference plus the F32_EVAL allowance of tests/test_gpu_batchnorm.py on the terms
    of z (its _check_elementwise, as it stands).
    f32 output (a case this file adds): there the storage ulp is the f32 ulp and the same bound, ulp(ref) + F32_EVAL * terms(z), was
    seen to FAIL on MI355X at the first tiling in every mode: for |z| <= 1/64 it allows little more than one f32 ulp at 0.5, while the
    evaluation rounds e = expf(-z) (<= 2 ulp), the sum 1 + e (half an ulp of a value in [1, 2]: 6e-8 whatever |z| is) and the
    division.  The sum's terms are e AND the constant 1, so the bound asserted is ulp(ref) + F32_EVAL * (terms(z) + 1); the observed
    share of both bounds is printed."""
    from test_gpu_batchnorm import F32_EVAL, _check_elementwise, _f32ulp
    s = P.FEATURE_SHAPES[1]
    for out in ("16", "f32"):
        rig = Rig(s, mode, out, act=R.SIGMOID, seed=70)
        z_terms = (rig.r.acc * rig.c.scale[:s.cout]).abs() + rig.c.shift[:s.cout].abs()
        share = {"z": 0.0, "z+1": 0.0}

        def check(t, rig=rig, out=out):
            rig.launch(t)
            got = rig.body()[..., :s.cout].double().cpu()
            if mode == "bf16x3" and out == "16":
                got = got + rig.body()[..., 2 * rig.Ct:2 * rig.Ct + s.cout].double().cpu()
            ref = rig.r.y[..., :s.cout]
            if out == "16":
                _check_elementwise(mode, got, ref, z_terms, f"sigmoid {t}")
            else:
                err = (got - ref).abs()
                share["z"] = max(share["z"], float((err / (_f32ulp(ref) + F32_EVAL * z_terms)).max()))
                share["z+1"] = max(share["z+1"], float((err / (_f32ulp(ref) + F32_EVAL * (z_terms + 1.0))).max()))
                assert bool((err <= _f32ulp(ref) + F32_EVAL * (z_terms + 1.0)).all()), f"sigmoid f32 {t}"
            sent = rig.body()[..., s.cout:rig.Ct]
            assert bool(torch.isnan(sent).all()), "write behind cout_store"
        n = rig.run_all(check=check)
        if out == "f32":
            print(f"[conv-tilings] sigmoid f32 {mode}: {n} pairs, worst share of ulp + F32_EVAL * terms(z): {share['z']:.3f}, "
                  f"of ulp + F32_EVAL * (terms(z) + 1): {share['z+1']:.3f}")


# ------------------------------------------------------------------------------------------------ temporal taps, reflection-pad fold
class pin_engine_launches:
    """While active, every sos_conv2d_fwd the engine issues for a descriptor `match` selects runs under a PINNED tiling: the first
    one select() offers for its shape whose geometry kind is in `kinds`.  The descriptors are the ones engine.conv fills (the
    existing tests' code paths); `pinned` records (kind, tiling) per launch."""

    def __init__(self, pinner, match, kinds):
        self.pinner, self.match, self.kinds, self.pinned = pinner, match, kinds, []

    def __enter__(self):
        h = self.pinner.h
        self.orig = h.sos_conv2d_fwd

        def launch(dref, stream):
            d = dref._obj
            if self.match(d):
                tl = [t for t in P.select(P.offered(self.pinner, d)) if t[4] in self.kinds and P.runs_as_pinned(d, t[3])]
                assert tl, f"no tiling of kind {self.kinds} is offered for {P.shape_key(d)}"
                self.pinner.pin(d, *tl[0][:4])
                self.pinned.append(tl[0])
            return self.orig(dref, stream)
        h.sos_conv2d_fwd = launch
        return self

    def __exit__(self, *exc):
        self.pinner.h.sos_conv2d_fwd = self.orig


NPOT_KINDS = ("npot", "npot-odd", "classes-npot", "classes3")
TILE_KINDS = {"npot": NPOT_KINDS, "multi-class": ("classes",)}


@pytest.mark.parametrize("kind", sorted(TILE_KINDS))
def test_temporal_taps_under_pinned_tilings(kind, mode):
    """Temporal taps (the table staging path: a chunk's offset moves by whole frames) under a non-power-of-two and a multi-class
    tile, neither of which the cost model picks for the shapes of test_gpu_train_ops.py's temporal test.  Same reference and
    tolerances as that test's forward part -- nn.Conv3d on the storage-rounded input, clips of 4 frames so that most frames touch
    the temporal padding -- on a layer of its own (48 -> 40 channels, horizontal dilation 2; the table is process-global)."""
    import torch.nn.functional as F
    from sos_amd import engine as E, _lib as L, train_ops as TO
    from test_gpu_train_ops import _act_to_nchw, _frames_act
    from util import hashed, rel_err
    x3 = mode == "bf16x3"
    B, T, I, O, H, W, kt = 2, 4, 48, 40, 15, 24, 3
    x = torch.from_numpy(hashed(91, (B, I, T, H, W)).astype(np.float32))
    xa, xheld = _frames_act(x, x3)
    w = torch.from_numpy((0.05 * hashed(92, (O, I, kt, 3, 3))).astype(np.float32))
    y = F.conv3d(xheld, w, None, 1, (1, 1, 2), (1, 1, 2))
    wp = E.pack_weight(w.permute(0, 2, 1, 3, 4).reshape(O, kt * I, 3, 3).cuda(), kt * I, x3)
    one, zero = TO.ones_zeros(wp.shape[1], torch.device("cuda"))
    dst = E.Act(B * T, H, W, 48, x3, torch.device("cuda"), zero=True)
    with pin_engine_launches(pinner_of(mode), lambda d: d.t_taps > 1, TILE_KINDS[kind]) as pins:
        E.conv_to_act(xa, 0, I, wp, 3, 3, O, one, zero, L.ACT_NONE, dst, cout_store=48, dil=(1, 2), pad=(1, 2), Ho=H, Wo=W, temporal=(T, kt))
    assert len(pins.pinned) == 1
    got = _act_to_nchw(dst, O).reshape(B, T, O, H, W).permute(0, 2, 1, 3, 4)
    e = rel_err(got, y)
    print(f"[conv-tilings] temporal taps {mode} {pins.pinned[0]}: rel err {e:.2e}")
    assert e < (3e-5 if x3 else 1e-2)


@pytest.mark.parametrize("kind", sorted(TILE_KINDS))
def test_reflection_pad_fold_under_pinned_tilings(kind, mode):
    """The reflection-pad fold of the data gradient (interior cells straight to the gradient tensor, border cells through the
    padded scratch tensor: the out2 branch of the staged store) under a non-power-of-two and a multi-class tile: the body,
    reference and bounds of test_gpu_train_ops.py::test_down_block_input_gradient (torch autograd; the computed storage-model
    bound in the 16-bit modes), stored and accumulated, on a block of its own (64 -> 128 channels, 3x3 at dilation 3: no network
    and no other test has a layer of dilation 3, and the table is process-global)."""
    from test_gpu_train_ops import test_down_block_input_gradient as body
    with pin_engine_launches(pinner_of(mode), lambda d: d.fold_pad > 0, TILE_KINDS[kind]) as pins:
        body((64, 128, 3, 1, 3, 22, 26), kind == "multi-class", mode == "bf16x3")
    assert len(pins.pinned) == 1, pins.pinned
    print(f"[conv-tilings] reflection-pad fold {mode} {pins.pinned[0]}")


# ------------------------------------------------------------------------------------------------ d. random-valued inputs
def _random_input(idx, shape, mode):
    from util import hashed
    return torch.from_numpy(hashed(idx, shape)).double()


def _random_weight(idx, shape, mode):
    from util import hashed
    return torch.from_numpy(hashed(idx, shape, 0.1)).double()


def test_random_valued_inputs_within_the_derived_bound(mode):
    """Realistic magnitudes (inputs U(-1, 1), weights U(-0.1, 0.1), rounded to storage; raw accumulators out): for every tiling of
    the 96 -> 96 shape |got - ref| <= (n_terms + 2) 2^-24 sum |w||x| on the f32 output -- any order of an f32 summation of n_terms
    exact products -- plus 1 storage ulp at the reference on the 16-bit output.  Prints the largest share of the bound used."""
    from test_gpu_batchnorm import _ulp
    s = {x.name: x for x in P.PLAIN_SHAPES}["5x5d(1,2) 96->96"]
    worst = {}
    for out in ("f32", "16"):
        rig = Rig(s, mode, out, act=R.NONE, epilogue=None, gen=(_random_input, _random_weight), exact=False, seed=80)
        ref = rig.r.y
        bound = R.random_bound(rig.r)
        if out == "16":
            bound = bound + _ulp(ref, mode)
        assert float(bound.min()) > 0

        def check(t, rig=rig, out=out, ref=ref, bound=bound):
            rig.launch(t)
            b = rig.body()
            got = b[..., :s.cout].double().cpu()
            if mode == "bf16x3" and out == "16":
                got = got + b[..., 2 * rig.Ct:2 * rig.Ct + s.cout].double().cpu()
            share = float(((got - ref).abs() / bound).max())
            worst[out] = max(worst.get(out, 0.0), share)
            assert share <= 1.0, f"random {out} {t}: {share:.3f} of the bound"
            assert bool(torch.isnan(b[..., s.cout:rig.Ct].float()).all())
        n = rig.run_all(check=check)
        print(f"[conv-tilings] random {mode} out={out}: {n} pairs, worst share of the bound {worst[out]:.3e}")
