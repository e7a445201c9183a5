"""Pin any legal plan of the weight-gradient kernels for a shape, inside one process, and ask the library what a descriptor
resolves to (tests/test_wgrad_plans_host_cpu.py, tests/test_gpu_wgrad_plans.py).

A PLAN of the tiled route is (MT, NTB, log2 NC, log2 TH, pixel order, workgroups per CU); log2 TW = 8 - log2 NC - log2 TH.
sos_wgrad_tune_load accepts a table line exactly when wg_make_plan() (csrc/wgrad.hip) offers that plan for the line's shape, and it
overwrites the table's entry of the shape.  So: write a one-line table, load it (1: offered, 0: not), ask sos_wgrad_describe (host
only, launches nothing) whether the descriptor now resolves to that plan, launch.  No legality rule is copied here: offered() loads
the full product of plan values and keeps what the library accepts.

The table is process-global and pins persist, and its 12-int key (Hg, Wg, kh, kw, stride, dil_h, dil_w, M, N, 16x16x32 kernel,
temporal taps, flat) has no batch, padding or Hx.  Every geometry below is therefore one that no line of the shipped
wgrad_table_gfx950.txt, no network and no other test uses (assert_not_shipped(); G images of 23 x 29, 17 x 23 under stride 2, 12 x 15,
5 x 7, 6 x 7 and flattened rows of 2 * 23 * 29 pixels)."""
import ctypes as C
import itertools
import os
import tempfile
from dataclasses import dataclass
from typing import Optional

HEADER = "sos_wgrad_tune 1 nkey 12\n"
FORCING = ("SOS_WGRAD_TILE", "SOS_WGRAD_MT", "SOS_WGRAD_NTB", "SOS_WGRAD_OCC")
ROUTES = ("gemm", "thin", "thin taps", "tiled")                  # out[0] of sos_wgrad_describe
KINDS = ("wgrad", "wgrad16", "thin", "thin_taps", "gemm")        # out[1]
EINVAL, ENOSPC = -22, -28                                       # SOS_EINVAL / SOS_ENOSPC
# the full product a table line can name (wg_make_plan's own bounds are narrower or equal: it is asked about every one)
PLAN_SPACE = list(itertools.product(range(1, 4), range(1, 5), range(0, 7), range(0, 9), (0, 1), range(1, 5)))


def forcing_switch():
    """The reason this process cannot pin plans, or None."""
    for name in FORCING:
        if os.environ.get(name) is not None:
            return name + " is set: the forced knobs bypass the plan table"
    if os.environ.get("SOS_WGRAD_TUNE_CACHE"):
        return "SOS_WGRAD_TUNE_CACHE is set: a user table is laid over the pins' shapes"
    from sos_amd import engine
    if engine.AUTOTUNE:
        return "SOS_CONV_TUNE=1: the autotuner owns the plan table"
    return None


@dataclass(frozen=True)
class Shape:
    """Geometry of one test gradient.  G is B images of Hg x Wg with M channels, X has N channels; 'same' padding
    (k - 1) / 2 * dil and Hx = (Hg - 1) * stride + 1 unless given."""
    name: str
    M: int
    N: int
    k: tuple
    dil: tuple = (1, 1)
    stride: int = 1
    reflect: bool = False
    Hg: int = 23
    Wg: int = 29
    B: int = 2
    pad: Optional[tuple] = None
    Hx: Optional[int] = None
    Wx: Optional[int] = None
    temporal: Optional[tuple] = None              # (frames per clip, taps, channels per frame)

    @property
    def padding(self):
        return self.pad if self.pad is not None else ((self.k[0] - 1) // 2 * self.dil[0], (self.k[1] - 1) // 2 * self.dil[1])

    @property
    def x_hw(self):
        return (self.Hx if self.Hx else (self.Hg - 1) * self.stride + 1, self.Wx if self.Wx else (self.Wg - 1) * self.stride + 1)

    @property
    def n_x(self):
        """channels of X a pixel stores for this gradient (temporal taps: one frame's)"""
        return self.temporal[2] if self.temporal else self.N

    @property
    def npix(self):
        return self.B * self.Hg * self.Wg


def pad16(n):
    return (n + 15) // 16 * 16


OFF = 8            # first owned channel of both operands in the descriptor tests


def layout(s):
    """(g_cs, g_off, x_cs, x_off) of the dense test operands: a non-zero offset, the owned run padded to whole 16-channel
    sub-images (what the streaming routes require of a pixel's channel run), eight more channels behind it."""
    return (OFF + pad16(s.M) + 8, OFF, OFF + pad16(s.n_x) + 8, OFF)


def geometry_desc(s, lay=None):
    """The sos_wgrad_desc of shape `s` without pointers (scale 1, automatic split)."""
    from sos_amd import _lib as L
    g_cs, g_off, x_cs, x_off = lay or layout(s)
    d = L.WgradDesc()
    d.B, d.Hg, d.Wg, d.g_cs, d.g_off = s.B, s.Hg, s.Wg, g_cs, g_off
    d.Hx, d.Wx, d.x_cs, d.x_off = s.x_hw[0], s.x_hw[1], x_cs, x_off
    d.M, d.N, d.kh, d.kw, d.stride, d.dil_h, d.dil_w = s.M, s.N, s.k[0], s.k[1], s.stride, s.dil[0], s.dil[1]
    d.pad_top, d.pad_left, d.pad_mode = s.padding[0], s.padding[1], 1 if s.reflect else 0
    d.ksplit, d.scale = 0, 1.0
    if s.temporal:
        T, kt, tcin = s.temporal
        d.t_frames, d.t_taps, d.t_pad, d.t_cin = T, kt, (kt - 1) // 2, tcin
    return d


_DUMMY = (C.c_float * 64)()


def with_dummy_pointers(d):
    """Host-only use (sos_wgrad_describe): non-null pointers that are never dereferenced."""
    p = C.cast(_DUMMY, C.c_void_p).value
    for f in ("g", "x", "partial", "dw"):
        if not getattr(d, f):
            setattr(d, f, p)
    return d


@dataclass(frozen=True)
class Info:
    """What sos_wgrad_describe reports (include/sos_hip.h)."""
    route: str
    kind: str
    a: int
    b: int
    v: int
    ksplit: int
    grid: int
    lds: int
    mt: int
    ntb: int
    nc: int
    lth: int
    ltw: int
    order: int
    occ: int
    dbuf: int
    xcdmap: int
    ntg: int
    nsteps: int

    @property
    def instance(self):
        return (self.kind, self.a, self.b, self.v)

    @property
    def plan(self):
        """the table-line form (MT, NTB, log2 NC, log2 TH, order, workgroups per CU)"""
        return (self.mt, self.ntb, self.nc.bit_length() - 1, self.lth, self.order, self.occ)


def describe(h, d):
    """(rc, Info or None) of a descriptor; pointers may be null (dummies are put in)."""
    from sos_amd import _lib as L
    out = (C.c_int32 * L.WGRAD_DESCRIBE_N)()
    rc = h.sos_wgrad_describe(C.byref(with_dummy_pointers(d)), out, L.WGRAD_DESCRIBE_N)
    if rc:
        return rc, None
    v = list(out)
    return 0, Info(ROUTES[v[0]], KINDS[v[1]], *v[2:])


def shape_key(h, d):
    """The 12 ints of a table line for the descriptor's shape (WgKey of wgrad.hip).  A congruent 1x1 gradient is keyed by its
    flattened row; whether the 16x16x32 kernel owns the shape is the library's answer (sos_wgrad_describe), not a rule copied here."""
    flat = (d.t_taps <= 1 and d.kh == 1 and d.kw == 1 and d.stride == 1 and d.pad_top == 0 and d.pad_left == 0 and d.Hg == d.Hx and
            d.Wg == d.Wx)
    rc, info = describe(h, d)
    assert rc == 0 and info.route == "tiled", (rc, info, h.sos_last_error().decode())
    Hg, Wg = (1, d.B * d.Hg * d.Wg) if flat else (d.Hg, d.Wg)
    return (Hg, Wg, d.kh, d.kw, d.stride, d.dil_h, d.dil_w, d.M, d.N, 1 if info.kind == "wgrad16" else 0,
            d.t_taps if d.t_taps > 1 else 0, 1 if flat else 0)


class Pinner:
    """One library handle and one scratch table file."""

    def __init__(self, h=None):
        from sos_amd import _lib as L, engine as E
        self.h = L.lib() if h is None else h
        if h is None:
            E._load_tune_cache()                  # the shipped table first: a later engine.wgrad would otherwise load it behind the pins
        fd, self.path = tempfile.mkstemp(prefix="sos_wgpin_", suffix=".txt")
        os.close(fd)
        self._default, self._offered, self._keys = {}, {}, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if os.path.exists(self.path):
            os.remove(self.path)

    def key(self, d):
        """shape_key(d); the first call for a shape also records the plan the cost model gives it (default_plan), because a pin
        cannot be taken back."""
        ident = (d.B, d.Hg, d.Wg, d.Hx, d.Wx, d.kh, d.kw, d.stride, d.dil_h, d.dil_w, d.M, d.N, d.t_taps, d.pad_top, d.pad_left)
        if ident not in self._keys:
            k = shape_key(self.h, d)
            self._keys[ident] = k
            if k not in self._default:
                self._default[k] = describe(self.h, d)[1].plan
        return self._keys[ident]

    def default_plan(self, d):
        """The plan the descriptor's shape had before anything was pinned for it (the cost model's)."""
        return self._default[self.key(d)]

    def load(self, key, mt, ntb, lnc, lth, kord, occ):
        """Load the one-line table: 1 if wg_make_plan() offers the plan for the shape (it is then the shape's entry), else 0."""
        with open(self.path, "w") as f:
            f.write(HEADER + " ".join(str(v) for v in key) + f" {mt} {ntb} {lnc} {lth} {kord} {occ}\n")
        return self.h.sos_wgrad_tune_load(self.path.encode())

    def pin(self, d, plan):
        """Make `plan` the plan of d's next launch -- or fail: the line must load and sos_wgrad_describe must report that very plan
        for the descriptor.  A pin that did not take effect is a failure, not a silent pass on another plan.  Returns the Info."""
        key = self.key(d)
        assert self.load(key, *plan) == 1, f"plan {plan} is not offered for shape {key}"
        rc, info = describe(self.h, d)
        assert rc == 0 and info.route == "tiled" and info.plan == tuple(plan) and info.ltw == 8 - plan[2] - plan[3], \
            f"pinned {plan} for shape {key}: the descriptor resolves to {info} (rc {rc}: {self.h.sos_last_error().decode()})"
        return info

    def load_lines(self, key, plans):
        """Load one table of several lines for the same shape: the number the library accepts (the last accepted stays pinned)."""
        with open(self.path, "w") as f:
            f.write(HEADER + "".join(" ".join(str(v) for v in key + tuple(p)) + "\n" for p in plans))
        return self.h.sos_wgrad_tune_load(self.path.encode())

    def offered(self, d):
        """Every plan of PLAN_SPACE the library accepts for d's shape (host only; leaves the last one pinned).  Cached.  The product is
        asked in blocks of one (MT, NTB, log2 NC) each; only a block of which the library accepts some line is asked line by line."""
        key = self.key(d)
        if key not in self._offered:
            got = []
            for _, block in itertools.groupby(PLAN_SPACE, key=lambda p: p[:3]):
                block = list(block)
                n = self.load_lines(key, block)
                if n:
                    mine = [p for p in block if self.load(key, *p) == 1]
                    assert len(mine) == n, (key, block[0][:3], n, mine)
                    got += mine
            self._offered[key] = got
        return self._offered[key]


def shipped_keys():
    from sos_amd import engine as E
    keys = set()
    for ln in open(E.SHIPPED_WGRAD_TABLE).read().splitlines()[1:]:
        v = ln.split()
        if len(v) >= 18:
            keys.add(tuple(int(x) for x in v[:12]))
    return keys


# (Hg, Wg, stride) of the G images the other weight-gradient tests launch (tests/test_gpu_train_ops.py; flattened 1x1 rows as
# (1, pixels, 1)); the networks' images are 256, 128 or 64 rows.  The shapes below stay clear of all of them.
ELSEWHERE = {(20, 40, 1), (33, 35, 1), (18, 21, 1), (9, 12, 2), (9, 21, 2), (1, 154, 1), (12, 19, 1), (15, 22, 2), (17, 23, 1),
             (37, 50, 1), (30, 41, 1), (21, 35, 1), (64, 45, 1), (40, 51, 1), (70, 81, 1), (37, 45, 1), (40, 37, 1), (9, 11, 2),
             (9, 11, 1), (5, 6, 2), (20, 33, 1), (23, 40, 1)}


def assert_not_shipped(pinner, shapes):
    """No pinned geometry may be a key of the shipped plan table, nor the G image of another test or of a network."""
    keys = shipped_keys()
    for s in shapes:
        k = pinner.key(geometry_desc(s))
        assert k not in keys, f"test shape {s.name}: {k} is a key of the shipped plan table"
        assert (k[0], k[1], k[4]) not in ELSEWHERE and k[0] not in (256, 128, 64), f"test shape {s.name}: image {k[:2]} is used elsewhere"


# ------------------------------------------------------------------------------------------------ the shapes
S = Shape
TILED_SHAPES = [
    S("5x5 96->96", 96, 96, (5, 5)),                                     # MT 1..3, both balanced instances (and their plain twins)
    S("5x5 64->96", 64, 96, (5, 5)),
    S("3x3 128->128", 128, 128, (3, 3)),                                 # NTB 1..3
    S("3x3 70->100", 70, 100, (3, 3)),                                   # ragged M and N tiles
    S("7x1 96->96", 96, 96, (7, 1)),
    S("1x1 100->200 flat", 100, 200, (1, 1)),                            # the flat tiled route; NTB 4, several workgroups per CU
    S("3x3 s2 reflect 64->128", 64, 128, (3, 3), stride=2, reflect=True, Hg=17, Wg=23),
    S("5x5 s2 reflect 128->64", 128, 64, (5, 5), stride=2, reflect=True, Hg=17, Wg=23),
    S("convT 3x3 s2 p1 64->32", 64, 32, (3, 3), stride=2, Hg=12, Wg=15, pad=(1, 1), Hx=24, Wx=30),      # role swap: G 12x15, X 24x30
    S("5x5 d(4,4) 96->96", 96, 96, (5, 5), (4, 4)),                      # NC 1, 2, 4
    S("5x5 d(2,3) 96->96", 96, 96, (5, 5), (2, 3)),                      # three class groups of NC = 1
    S("5x5 d(32,32) 96->96", 96, 96, (5, 5), (32, 32)),                  # dilation beyond the image: whole classes and tiles outside
    S("5x5 96->96 on 5x7", 96, 96, (5, 5), Hg=5, Wg=7),                  # smaller than every tile
    S("3x3 2->64 narrow", 2, 64, (3, 3)),
    S("7x7 s2 128->16", 128, 16, (7, 7), stride=2, Hg=17, Wg=23),        # two tap-row groups, the last with a phantom row
    S("7x7 s1 48->32", 48, 32, (7, 7)),
    S("16: 5x5 48->48", 48, 48, (5, 5)),
    S("16: 5x5 d(4,4) 48->40", 48, 40, (5, 5), (4, 4)),
    S("16: 3x3 reflect 40->48", 40, 48, (3, 3), reflect=True),
    S("16: 7x1 48->48", 48, 48, (7, 1)),
    S("temporal 3x3 kt3 32<-128", 32, 384, (3, 3), Hg=6, Wg=7, B=8, temporal=(4, 3, 128)),
]
GEMM_SHAPES = [S("gemm 160x256 over 77", 160, 256, (1, 1), Hg=1, Wg=77, B=1),
               S("gemm 288x416 over 2x7x331", 288, 416, (1, 1), Hg=7, Wg=331, B=2)]
# one (M, N) per compiled (m16, n16) of the thin 1x1 streaming kernel x three pixel counts
THIN_MN = [(14, 10), (30, 14), (48, 14), (64, 10), (96, 14), (8, 30), (8, 48), (4, 64), (8, 96)]
THIN_PIX = [(1, 1, 20), (1, 37, 50), (2, 37, 60)]                       # waves with empty runs; one workgroup; two workgroups
THIN_SHAPES = [S(f"thin {m}x{n} over {b}x{hh}x{ww}", m, n, (1, 1), Hg=hh, Wg=ww, B=b) for m, n in THIN_MN for b, hh, ww in THIN_PIX]
TAPS_SHAPES = [S(f"taps {m}x{n} {nm}", m, n, (5, 1), (dl, 1), reflect=rf, Hg=5, Wg=33, pad=(pd, 0))
               for m in (49, 56, 64) for n in (10, 16) for nm, rf, dl, pd in (("reflect", True, 1, 2), ("zero", False, 1, 2), ("dil2", False, 2, 4))]
ROUTE_SHAPES = GEMM_SHAPES + THIN_SHAPES + TAPS_SHAPES
ALL_SHAPES = TILED_SHAPES + ROUTE_SHAPES

# the expected contents of wg_instances (csrc/wgrad.hip): (kernel kind, a, b, v)
INSTANCES = ([("wgrad", mt, ntb, 0) for mt in (1, 2, 3) for ntb in (1, 2, 3, 4)] + [("wgrad", 3, 1, 1), ("wgrad", 2, 1, 1)] +
             [("wgrad16", 3, 3, 3), ("wgrad16", 3, 3, 1)] +
             [("thin", m, 1, 0) for m in (1, 2, 3, 4, 6)] + [("thin", 1, n, 0) for n in (2, 3, 4, 6)] +
             [("thin_taps", 4, 5, 0), ("gemm", 0, 0, 0)])
# compiled instances no shape can reach, each with the reason (none: every entry of wg_instances is reached by a shape above)
DEAD_INSTANCES = {}


def variants(infos):
    """The subset of a shape's plans that also runs the descriptor variants (accumulate, scale, explicit ksplit, partial + reduce):
    for every kernel instance the first and the last plan offered, and the first plan with each feature (dbuf 0 / 1, order 0 / 1,
    NC > 1, several workgroups per CU).  infos: [(plan, Info)] -> set of plans."""
    pick = {}
    for plan, i in infos:
        for feat in (("first", i.instance), ("dbuf", i.dbuf), ("order", i.order), ("nc", i.nc > 1), ("occ", i.occ > 1)):
            pick.setdefault(feat, plan)
        pick[("last", i.instance)] = plan
    return set(pick.values())
