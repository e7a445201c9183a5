"""Pin any legal tiling of the forward convolution for a shape, inside one process (tests/test_conv_tilings_host_cpu.py,
tests/test_gpu_conv_tilings.py).

sos_conv2d_tune_load accepts a table entry if and only if enumerate_cfgs() (csrc/conv.hip) offers that tiling for the entry's
shape, and overwrites the table's entry for the shape.  So: write a one-line table, load it (1: offered, 0: not), launch.  The
table is process-global and pins persist: the shapes below use geometries no network, no other test and no line of the shipped
table uses (assert_not_shipped()).

A tiling is (NC, TH, TW, ks): NC residue classes of the horizontal dilation x TH x TW strided pixels, and the kernel-instance code
`ks` of the table's file format (comment above struct KsCode in conv.hip): 0 / -1 the 16-row kernel with two / one slab buffers,
1..8 k-steps of the 32-row kernel, + 100 one weight-slab buffer, + 200 three workgroups per CU, + 300 the 384-slot tile,
+ 1000 nt: nt n-tiles per workgroup instead of nt_for()."""
import ctypes as C
import os
import sys
import tempfile
from dataclasses import dataclass

HEADER = "sos_conv_tune 2 abi 3 nkey 19\n"
DT = {"bf16": 0, "fp16": 0, "bf16x3": 1}         # SOS_DT_* of a 16-bit output in each storage mode
DT_F32 = 2
FORCING = ("SOS_CONV_FORCE_CFG", "SOS_CONV_FORCE_PT3", "SOS_CONV_FORCE_W3", "SOS_CONV16_MODE")
KSTEPS = (1, 2, 3, 4, 5, 6, 8)
# every ks code of the file format this build could name: the 16-row kernel's two, then each k-step count plain, single slab, three
# per CU, 384-slot, and as two n-blocks of 64 output channels
KS_CODES = (0, -1) + tuple(k + m for k in KSTEPS for m in (0, 100, 200, 300, 2000))


def forcing_switch():
    """The reason this process cannot pin tilings (a forcing switch takes precedence over the table), or None."""
    for name in FORCING:
        if os.environ.get(name) is not None:
            return name + " is set: forcing switches take precedence over the tiling table"
    from sos_amd import engine
    if engine.AUTOTUNE:
        return "SOS_CONV_TUNE=1: the autotuner owns the tiling table"
    return None


@dataclass(frozen=True)
class Shape:
    """Geometry of one test convolution: 'same' padding (k - 1) / 2 * dil, B images of H x W."""
    name: str
    cin: int
    cout: int
    k: tuple
    dil: tuple = (1, 1)
    stride: int = 1
    reflect: bool = False
    H: int = 23
    W: int = 29
    B: int = 2

    @property
    def pad(self):
        return ((self.k[0] - 1) // 2 * self.dil[0], (self.k[1] - 1) // 2 * self.dil[1])

    @property
    def Ho(self):
        return (self.H + 2 * self.pad[0] - self.dil[0] * (self.k[0] - 1) - 1) // self.stride + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pad[1] - self.dil[1] * (self.k[1] - 1) - 1) // self.stride + 1

    @property
    def cout_pad(self):
        return (self.cout + 31) // 32 * 32


def geometry_desc(s, mode, out="16", Wl=None, gather=False):
    """The sos_conv_desc engine.conv would fill for shape `s` in storage mode `mode`, without pointers: out = '16' (dense NHWC in
    the storage type, hi|hi|lo in bf16x3), 'f32' (dense f32 NHWC) or 'f32s' (f32, out_sc != 1).  The caller adds buffers."""
    from sos_amd import _lib as L
    d = L.ConvDesc()
    nseg = 3 if mode == "bf16x3" else 1
    d.B, d.H, d.W = s.B, s.H, s.W
    d.in_cs, d.cin_off, d.cin, d.in_nseg, d.in_seg_stride = nseg * s.cin, 0, s.cin, nseg, s.cin
    d.Wl = s.W if Wl is None else Wl
    d.kh, d.kw, d.cout, d.cout_pad = s.k[0], s.k[1], s.cout, s.cout_pad
    d.stride, d.dil_h, d.dil_w = s.stride, s.dil[0], s.dil[1]
    d.pad_top, d.pad_left, d.pad_mode = s.pad[0], s.pad[1], 1 if s.reflect else 0
    d.Ho, d.Wo = s.Ho, s.Wo
    d.cout_store = s.cout
    if out == "16":
        row = nseg * s.cout_pad
        d.out_dtype, d.out_sc, d.out_sw, d.out_third = DT[mode], 1, row, s.cout_pad
    else:
        d.out_dtype, d.out_sc, d.out_sw = DT_F32, (1 if out == "f32" else s.Ho * s.Wo), (s.cout_pad if out == "f32" else 1)
    if out == "f32s":
        d.out_sh, d.out_sb = s.Wo, s.Ho * s.Wo * s.cout_pad          # NCHW
    else:
        d.out_sh = s.Wo * d.out_sw
        d.out_sb = s.Ho * d.out_sh
    if gather:
        d.w_gather = 1                            # (a flag of the shape key; the caller puts the table's address here)
    return d


def with_dummy_pointers(d, keep):
    """Host-only use (sos_conv2d_tile_count): non-null pointers that are never dereferenced."""
    buf = (C.c_float * 64)()
    keep.append(buf)
    p = C.cast(buf, C.c_void_p).value
    d.in_, d.wgt, d.out = p, p, p
    for f in ("w_gather", "stats", "wl_tab", "wo_tab", "in_scale", "in_shift", "scale", "shift"):
        if getattr(d, f):
            setattr(d, f, p)
    return d


def nseg_eff(d):
    return d.in_nseg * (d.t_taps if d.t_taps > 1 else 1)


def shape_key(d):
    """The 19 ints of a table line (documented above sos_conv2d_tune_save; ShapeKey of conv.hip)."""
    return (d.B, d.H, d.W, d.Wl, d.cin, nseg_eff(d), d.cout_pad, d.kh, d.kw, d.stride, d.dil_h, d.dil_w, d.Ho, d.Wo, d.out_dtype,
            1 if d.out_sc == 1 else 0, d.pad_mode, 1 if d.w_gather else 0, d.cout)


def tenc(v):
    """Tile size as the file holds it: the log2 of a power of two, else the size + 16."""
    for l in range(16):
        if (1 << l) == v:
            return l
    return v + 16


def tdim(l):
    """... and back."""
    return 1 << l if l < 16 else l - 16


def nt_for(d):
    ntiles = d.cout_pad // 32
    nby = (ntiles + 3) // 4
    return (ntiles + nby - 1) // nby


def nt16_for(d):
    plain = d.in_nseg == 1 and d.out_dtype == 0
    x3 = d.in_nseg == 3 and d.out_dtype == 1
    if not (plain or x3) or d.t_taps > 1 or d.out_sc != 1 or d.cin not in (16, 48):
        return 0
    if d.cout <= 16:
        return 1
    return 3 if 32 < d.cout <= 48 else 0


def decode(ks, d):
    """(row16, nt, ks, nbuf, w3, slots): the kernel instance a ks code names for the descriptor (decode() of conv.hip)."""
    if ks <= 0:
        return (True, nt16_for(d), d.cin // 16, 2 if ks == 0 else 1, False, 256)
    nt = nt_for(d)
    if ks >= 1000:
        nt, ks = ks // 1000, ks % 1000
    m = ks // 100
    return (False, nt, ks % 100, 1 if m == 1 else 2, m == 2, 384 if m == 3 else 256)


def dense16(d):
    """plan()'s condition for the three-per-CU and the 384-slot instances: one 16-bit plane of whole 8-channel pieces."""
    return d.out_dtype == 0 and d.out_sc == 1 and nseg_eff(d) == 1 and d.cout_store % 8 == 0


def tile_count(d, NC, TH, TW):
    Hc, Wc = -(-d.Ho // d.dil_h), -(-d.Wo // d.dil_w)
    return d.B * d.dil_h * -(-Hc // TH) * -(-d.dil_w // NC) * -(-Wc // TW)


class Pinner:
    """One library handle and one scratch table file."""

    def __init__(self, h=None):
        from sos_amd import _lib as L, engine as E
        self.h = L.lib() if h is None else h
        if h is None:
            E._load_tune_cache()                  # the shipped table first: a later engine.conv would lay it over the pins
        fd, self.path = tempfile.mkstemp(prefix="sos_pin_", suffix=".txt")
        os.close(fd)
        self.keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if os.path.exists(self.path):
            os.remove(self.path)

    def load(self, key, NC, TH, TW, ks):
        """Load the one-line table: 1 if enumerate_cfgs() offers the tiling for the shape (it is then the shape's entry), else 0."""
        with open(self.path, "w") as f:
            f.write(HEADER + " ".join(str(v) for v in key) + f" {NC} {tenc(TH)} {tenc(TW)} {ks}\n")
        return self.h.sos_conv2d_tune_load(self.path.encode())

    def resolved(self, d):
        """(sos_conv2d_tile_count of the descriptor, what resolve() listed).  With SOS_CONV_LIST set the library names on stderr the
        candidate it takes from the COST-ORDERED LIST, i.e. when neither the table's entry nor a borrowed one ran: an empty text
        means the table's entry (or, for a three-per-CU entry plan() refuses, its plain twin) is what the next launch uses."""
        if not d.in_:
            d = with_dummy_pointers(d, self.keep)
        sys.stderr.flush()
        saved, had = os.dup(2), os.environ.get("SOS_CONV_LIST")
        with tempfile.TemporaryFile(mode="w+b") as tmp:
            os.dup2(tmp.fileno(), 2)
            os.environ["SOS_CONV_LIST"] = "1"
            try:
                n = self.h.sos_conv2d_tile_count(C.byref(d))
            finally:
                os.dup2(saved, 2)
                os.close(saved)
                if had is None:
                    del os.environ["SOS_CONV_LIST"]
                else:
                    os.environ["SOS_CONV_LIST"] = had
            tmp.seek(0)
            return n, tmp.read().decode()

    def pin(self, d, NC, TH, TW, ks):
        """Make (NC, TH, TW, ks) the tiling of d's next launch -- or fail: the entry must load, the descriptor must resolve to the
        table's entry and to the pinned tile count, and a three-per-CU entry must not have been swapped for its plain twin (plan()'s
        condition, mirrored by runs_as_pinned()).  A pin that did not take effect is a failure, not a silent pass on another
        tiling."""
        assert self.load(shape_key(d), NC, TH, TW, ks) == 1, f"tiling NC={NC} TH={TH} TW={TW} ks={ks} is not offered for this shape"
        (got, listed), want = self.resolved(d), tile_count(d, NC, TH, TW)
        assert got == want and not listed, (f"pinned NC={NC} TH={TH} TW={TW} ks={ks} ({want} tiles): the descriptor resolves to {got} "
                                            f"tiles, {listed.strip() or 'from the table'} ({self.h.sos_last_error().decode()})")
        assert runs_as_pinned(d, ks), f"ks={ks}: plan() refuses this instance for the descriptor (its plain twin would run)"
        return want


def runs_as_pinned(d, ks):
    """plan()'s descriptor conditions on the three-per-CU and 384-slot instances."""
    _, _, _, _, w3, slots = decode(ks, d)
    if w3:
        return dense16(d) and not d.accumulate
    if slots == 384:
        return dense16(d) and not d.wl_tab
    return True


def candidates(d, every_code=False):
    """A superset of the tilings enumerate_cfgs() can offer for d's shape: NC in the powers of two and {3, 6, 12, 24} up to
    dil_w, TH / TW in the powers of two, the equal-part cuts of the strided extent into 1..3 parts and the 384-slot widths and
    heights, every ks code of the file format.  Left out, to keep the number of loads small, is only what no rule of
    enumerate_cfgs() produces: tiles of fewer than 160 pixels, k-step counts that do not divide cin / 16, the 16-row codes where
    nt16_for() is 0, + 200 / + 300 without three n-tiles, + 2000 without four.  every_code=True keeps all ks codes: the host coverage
    test (test_conv_tilings_host_cpu.py) loads those for every shape, requires the same verdicts as the pruned list and asks the
    library about tiles below 160 pixels, so that nothing it asserts rests on the rules copied here."""
    Hc, Wc = -(-d.Ho // d.dil_h), -(-d.Wo // d.dil_w)
    ncs = sorted({n for n in [1 << l for l in range(9)] + [3, 6, 12, 24] if n <= max(1, d.dil_w)})
    pow2 = [1 << l for l in range(9)]
    ths = set(pow2) | {-(-Hc // p) for p in (1, 2, 3)} | {min(t, Hc) for t in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)}
    for t in list(ths):                           # the 384-slot rule's balanced heights
        ths.add(-(-Hc // -(-Hc // t)))
    nt = nt_for(d)
    codes = list(KS_CODES) if every_code else [k for k in KS_CODES if (k <= 0 and nt16_for(d)) or
             (k > 0 and (d.cin // 16) % (k % 100) == 0 and (k // 100 not in (2, 3) or nt == 3) and (k < 2000 or nt == 4))]
    out = []
    for NC in ncs:
        tws = set(pow2) | {-(-Wc // p) for p in (1, 2, 3)}
        for TH in ths:                            # the 384-slot rule's widths: the widest that fits, and its balanced cut
            if NC * TH <= 384:
                w = min(384 // (NC * TH), Wc, 64)
                if w >= 1:
                    tws.add(w)
                    tws.add(-(-Wc // -(-Wc // w)))
        for TH in sorted(ths):
            for TW in sorted(tws):
                if not 160 <= NC * TH * TW <= 384:
                    continue
                for ks in codes:
                    if NC * TH * TW > 256 and ks // 100 != 3:
                        continue
                    out.append((NC, TH, TW, ks))
    return out


_OFFERED = {}


def offered(pinner, d, every_code=False):
    """The candidates enumerate_cfgs() offers for d's SHAPE (host only; leaves the last one pinned).  Cached per library."""
    key = shape_key(d)
    if every_code:                                # (the host coverage test: no ks code is left out on the word of a Python rule)
        return [c for c in candidates(d, True) if pinner.load(key, *c) == 1]
    if (id(pinner.h), key) not in _OFFERED:
        _OFFERED[(id(pinner.h), key)] = [c for c in candidates(d) if pinner.load(key, *c) == 1]
    return _OFFERED[(id(pinner.h), key)]


def _pow2(v):
    return v & (v - 1) == 0


def kind_of(NC, TH, TW, ks):
    """The tile-geometry kind of a tiling (the kinds test_gpu_conv_tilings.py runs for every ks code)."""
    if ks > 0 and ks % 1000 // 100 == 3:
        return "slots384" if NC * TH * TW == 384 else "slots3xx"
    p2 = _pow2(TH) and _pow2(TW) and _pow2(NC)
    if NC == 1:
        if not p2:
            return "npot-odd" if TH % 2 and TW % 2 and TH > 1 else "npot"
        if TH == 1:
            return "row"
        if TW == 8:
            return "tw8"
        if TH >= 64:
            return "tall"
        return "pow2"
    if NC % 3 == 0:
        return "classes3"
    return "classes" if p2 else "classes-npot"


def select(tilings):
    """The cap on what a shape runs: for every ks code offered, one tiling of each geometry kind -- the most square tile of the
    kind (the tallest for 'tall'), ties by (NC, TH, TW).  Returns [(NC, TH, TW, ks, kind)]."""
    best = {}
    for (NC, TH, TW, ks) in tilings:
        kind = kind_of(NC, TH, TW, ks)
        score = (-TH if kind == "tall" else abs(TH - TW), NC, TH, TW)
        if (ks, kind) not in best or score < best[(ks, kind)][0]:
            best[(ks, kind)] = (score, (NC, TH, TW, ks, kind))
    return [v[1] for _, v in sorted(best.items())]


def shipped_keys():
    from sos_amd import engine as E
    keys = set()
    if os.path.exists(E.SHIPPED_TUNE_TABLE):
        for ln in open(E.SHIPPED_TUNE_TABLE).read().splitlines()[1:]:
            v = ln.split()
            if len(v) >= 23:
                keys.add(tuple(int(x) for x in v[:19]))
    return keys


def assert_not_shipped(descs):
    """No pinned shape may be a key of the shipped table, nor the same LAYER as one (tuned_borrow() hands a table entry to every
    other geometry of its layer: a pin must never become another test's tiling, nor a shipped entry a pinned shape's)."""
    keys = shipped_keys()
    layers = {layer_of(k) for k in keys}
    for d in descs:
        k = shape_key(d)
        assert k not in keys, f"test shape {k} is a key of the shipped tiling table"
        assert layer_of(k) not in layers, f"test shape {k} is a layer of the shipped tiling table"


def layer_of(key):
    """The fields of a key tuned_borrow() matches a layer by (everything but B, H, W, Wl, Ho, Wo)."""
    return tuple(key[i] for i in (4, 5, 6, 7, 8, 9, 10, 11, 14, 15, 16, 17, 18))


# ------------------------------------------------------------------------------------------------ the shapes
# H and W are primes or odd numbers no network produces (the networks' images are 256 rows or one row); every (cin, cout, kernel,
# dilation) combination is checked against the shipped table at import of the tests.
S = Shape
PLAIN_SHAPES = [
    # k-steps 1..8 (cin / 16) x n-tiles 1..4 (cout_pad / 32; 160: three n-tiles and a partial last n-block)
    S("5x5d(2,3) 80->21", 80, 21, (5, 5), (2, 3), H=23, W=26),
    S("5x5d(2,3) 96->29", 96, 29, (5, 5), (2, 3), H=23, W=26),
    S("5x5d(1,8) 128->27", 128, 27, (5, 5), (1, 8), H=13, W=37),
    S("3x3r 80->45", 80, 45, (3, 3), reflect=True, H=19, W=31),
    S("3x3r 96->61", 96, 61, (3, 3), reflect=True, H=19, W=31),
    S("5x5d(2,6) 128->53", 128, 53, (5, 5), (2, 6), H=21, W=40),
    S("5x5d(2,3) 80->91", 80, 91, (5, 5), (2, 3), H=23, W=26),
    S("5x5d(1,2) 96->96", 96, 96, (5, 5), (1, 2), H=39, W=33),
    S("3x3r 128->83", 128, 83, (3, 3), reflect=True, H=13, W=39),
    S("1x1 80->125", 80, 125, (1, 1), H=15, W=37),
    S("5x5d(2,6) 96->127", 96, 127, (5, 5), (2, 6), H=21, W=40),
    S("3x3r 128->123", 128, 123, (3, 3), reflect=True, H=13, W=39),
    # single slab with one and two n-tiles: patches whose tap-loop LDS crosses a third of the CU between one and two slab buffers
    # (one n-tile at one k-step: 972..1020 patch pixels -- no odd kernel has a power-of-two tile in that window; 6x5 taps over eight
    # classes of 2 x 16 pixels has 1008)
    S("6x5d(1,8) 16->30", 16, 30, (6, 5), (1, 8), H=13, W=37),
    S("3x3r 64->30", 64, 30, (3, 3), reflect=True, H=19, W=31),
    S("1x1 64->50", 64, 50, (1, 1), H=15, W=37),
    S("5x5d(1,8) 32->30", 32, 30, (5, 5), (1, 8), H=13, W=37),
    S("5x5d(1,8) 48->50", 48, 50, (5, 5), (1, 8), H=13, W=37),
    S("5x5d(1,8) 64->50", 64, 50, (5, 5), (1, 8), H=13, W=37),
    S("5x5d(1,8) 32->96", 32, 96, (5, 5), (1, 8), H=13, W=37),
    S("5x5d(2,3) 48->96", 48, 96, (5, 5), (2, 3), H=23, W=26),
    # a partial last n-block: cout_pad = 160 runs as n-blocks of 96 and 64 output channels
    S("3x3r 32->157", 32, 157, (3, 3), reflect=True, H=19, W=31),
    S("1x1 64->130", 64, 130, (1, 1), H=15, W=37),
    # the 16-row kernel: cout <= 16 and 33..48 with cin 16 / 48
    S("5x5d(2,3) 16->13", 16, 13, (5, 5), (2, 3), H=23, W=26),
    S("3x3r 48->15", 48, 15, (3, 3), reflect=True, H=19, W=31),
    S("5x5d(1,8) 16->45", 16, 45, (5, 5), (1, 8), H=13, W=37),
    S("5x5d(2,3) 48->45", 48, 45, (5, 5), (2, 3), H=23, W=26),
]
# DownConvBlock: ReflectionPad2d(2) + Conv2d(k = 5, stride 2), odd H and W
STRIDE2_SHAPES = [S("5x5s2r 64->60", 64, 60, (5, 5), stride=2, reflect=True, H=27, W=35),
                  S("5x5s2r 48->45", 48, 45, (5, 5), stride=2, reflect=True, H=27, W=35)]
# descriptor features: three n-tiles (three per CU and 384-slot tiles exist) at two and three k-steps; cout < cout_pad leaves room for
# cout_store > cout inside the padded channel count
FEATURE_SHAPES = [S("5x5d(2,3) 96->88 f", 96, 88, (5, 5), (2, 3), H=25, W=34),
                  S("3x3r 48->88 f", 48, 88, (3, 3), reflect=True, H=21, W=43)]
ALL_SHAPES = PLAIN_SHAPES + STRIDE2_SHAPES + FEATURE_SHAPES

# every compiled instance without the fused input BatchNorm, (row16, nt, ks, nbuf, w3, slots): conv_instances of conv.hip
INSTANCES = ([(False, nt, ks, 2, False, 256) for nt in (1, 2, 3, 4) for ks in KSTEPS] +
             [(False, nt, ks, 1, False, 256) for nt in (1, 2, 3) for ks in (1, 2, 3, 4)] +
             [(False, 3, 1, 2, True, 256), (False, 3, 2, 2, True, 256), (False, 3, 2, 2, False, 384), (False, 3, 3, 2, False, 384)] +
             [(True, nt, ks, nbuf, False, 256) for nt in (1, 3) for ks in (1, 3) for nbuf in (2, 1)])
# compiled but never offered: enumerate_cfgs() adds a single-slab candidate of three n-tiles for ks <= 2 only (ks >= 3 spills at the
# 168-register limit of three waves per SIMD), yet SOS_K32_SINGLE(3) still builds ks 3 and 4
DEAD_INSTANCES = {(False, 3, 3, 1, False, 256): "single slab, three n-tiles, three k-steps: spills; enumerate_cfgs() never offers it",
                  (False, 3, 4, 1, False, 256): "single slab, three n-tiles, four k-steps: spills; enumerate_cfgs() never offers it"}
