"""Host-side checks (no GPU) of what tests/test_gpu_wgrad_plans.py launches: sos_wgrad_describe resolves a descriptor -- route, kernel
instance, plan, split -- without launching, so the coverage of the GPU module, the refusals of wg_make_plan() / wg_route(), the
route boundaries and the forced knobs are all asked of the library here, on the CPU."""
import os
import re

import pytest

import wgrad_pin as P

if P.forcing_switch():
    pytest.skip(P.forcing_switch(), allow_module_level=True)


@pytest.fixture(scope="module")
def pinner():
    with P.Pinner() as pn:
        P.assert_not_shipped(pn, P.TILED_SHAPES)
        yield pn


def _source_instances():
    """wg_instances of csrc/wgrad.hip with its two macros expanded -> [(kind, a, b, v)]."""
    from sos_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "wgrad.hip")).read()
    body = re.search(r"static const WgInstance wg_instances\[\] = \{(.*?)\n\};", src, re.S).group(1)
    body = re.sub(r"SOS_WG32\((\d+), (\d+)\)", r"{k, WG_K32, \1, \2, 0}", body)
    body = re.sub(r"SOS_WGT\((\d+), (\d+)\)", r"{k, WG_KTHIN, \1, \2, 0}", body)
    names = {"WG_K32": "wgrad", "WG_K16": "wgrad16", "WG_KTHIN": "thin", "WG_KTAPS": "thin_taps", "WG_KGEMM": "gemm"}
    found = re.findall(r"(WG_K\w+), (\d+), (\d+), (\d+)\}", body)
    assert len(found) == body.count("WG_K"), "an entry of wg_instances was not parsed"
    return [(names[k], int(a), int(b), int(v)) for k, a, b, v in found]


def test_instance_list_is_the_one_the_tests_expect():
    """A new (or removed) kernel instance fails here until wgrad_pin.INSTANCES names it -- and then the coverage test below fails
    until a shape reaches it."""
    got = _source_instances()
    assert len(got) == len(set(got)) == 27
    assert sorted(got) == sorted(P.INSTANCES)
    assert set(P.DEAD_INSTANCES) <= set(P.INSTANCES)


def _all_infos(pn):
    """{shape name: [(plan or None, Info)]} of everything the GPU module launches with the default knobs."""
    out = {}
    for s in P.TILED_SHAPES:
        d = P.geometry_desc(s)
        out[s.name] = [(p, pn.pin(d, p)) for p in pn.offered(d)]
    for s in P.ROUTE_SHAPES:
        rc, info = P.describe(pn.h, P.geometry_desc(s))
        assert rc == 0, (s.name, pn.h.sos_last_error().decode())
        out[s.name] = [(None, info)]
    return out


def test_the_gpu_shape_list_reaches_every_instance_route_and_feature(pinner, monkeypatch):
    infos = _all_infos(pinner)
    flat = [i for v in infos.values() for _, i in v]
    assert len(flat) > 1500                       # the full product of offered plans: nothing is pruned
    reached = {i.instance for i in flat}
    assert reached == set(P.INSTANCES) - set(P.DEAD_INSTANCES), sorted(set(P.INSTANCES) - reached)
    assert {i.route for i in flat} == set(P.ROUTES)
    tiled = [i for i in flat if i.route == "tiled"]
    for feature, values in (("dbuf", {0, 1}), ("order", {0, 1}), ("xcdmap", {0, 1})):
        assert {getattr(i, feature) for i in tiled} == values, feature
    assert {1, 2, 4, 8, 16, 32} <= {i.nc for i in tiled}
    assert {1, 2} == {i.ntg for i in tiled}
    assert {1, 2, 3, 4} == {i.occ for i in tiled}
    assert {1, 2, 3} == {i.mt for i in tiled if i.kind == "wgrad"} and {1, 2, 3, 4} == {i.ntb for i in tiled if i.kind == "wgrad"}
    assert any(i.ksplit == i.nsteps for i in tiled) and any(i.ksplit < i.nsteps for i in tiled)      # ksplit clipped to nsteps, and not
    for i in tiled:
        assert 1 <= i.ksplit <= i.nsteps and i.grid % i.ksplit == 0 and i.lds <= 160 * 1024 // i.occ, i
    # per shape what the issue of this test module names
    def of(name, **want):
        return [i for _, i in infos[name] if all(getattr(i, k) == v for k, v in want.items())]
    for name in ("5x5 96->96", "5x5 64->96"):
        assert of(name, kind="wgrad", mt=2, v=1) and of(name, mt=1, v=0)
    assert of("5x5 96->96", mt=3, v=1)
    assert {i.ntb for _, i in infos["3x3 128->128"]} == {1, 2, 3} == {i.ntb for _, i in infos["7x1 96->96"]}
    assert {i.ntb for _, i in infos["1x1 100->200 flat"]} == {1, 2, 3, 4} and of("1x1 100->200 flat", occ=2)
    assert {i.nc for _, i in infos["5x5 d(4,4) 96->96"]} == {1, 2, 4} and {i.nc for _, i in infos["5x5 d(2,3) 96->96"]} == {1}
    assert all(i.ntg == 2 for n in ("7x7 s2 128->16", "7x7 s1 48->32") for _, i in infos[n])
    assert {i.instance for n, v in infos.items() if n.startswith("16:") for _, i in v} == {("wgrad16", 3, 3, 3), ("wgrad16", 3, 3, 1)}
    assert {i.instance for n, v in infos.items() if n.startswith("thin") for _, i in v} == {i for i in P.INSTANCES if i[0] == "thin"}
    assert {i.ksplit for n, v in infos.items() if n.startswith("thin") for _, i in v} == {1, 2}
    # the plain twins of the balanced instances
    monkeypatch.setenv("SOS_WGRAD_NOBAL", "1")
    d = P.geometry_desc(P.TILED_SHAPES[0])
    twins = {pinner.pin(d, p).instance for p in pinner.offered(d)}
    assert twins == {("wgrad", 1, 1, 0), ("wgrad", 2, 1, 0), ("wgrad", 3, 1, 0)}
    # SOS_WGG_SPLIT sets the GEMM's split
    monkeypatch.delenv("SOS_WGRAD_NOBAL")
    gemm77 = P.geometry_desc(P.GEMM_SHAPES[0])
    for split in (1, 2, 3):
        monkeypatch.setenv("SOS_WGG_SPLIT", str(split))
        assert P.describe(pinner.h, gemm77)[1].ksplit == split


def _shape_desc(M, N, k=(1, 1), **kw):
    return P.geometry_desc(P.Shape("probe", M, N, k, **kw))


def test_plans_the_library_refuses(pinner):
    """wg_make_plan(): more than 32 (tap, n-tile) pairs, classes that do not divide the dilation, classes under stride 2, more
    m-tiles than the shape has, LDS beyond the CU's share."""
    pn = pinner
    k55 = pn.key(P.geometry_desc(P.TILED_SHAPES[0]))                     # 5x5 96 -> 96
    assert pn.load(k55, 3, 1, 0, 4, 1, 1) == 1
    assert pn.load(k55, 3, 2, 0, 4, 1, 1) == 0                           # 2 n-tiles x 25 taps
    assert pn.load(k55, 3, 1, 1, 4, 1, 1) == 0                           # two classes at dilation 1
    k23 = pn.key(P.geometry_desc(next(s for s in P.TILED_SHAPES if s.name == "5x5 d(2,3) 96->96")))
    assert pn.load(k23, 3, 1, 1, 3, 1, 1) == 0                           # NC = 2 does not divide dil_w = 3
    k44 = pn.key(P.geometry_desc(next(s for s in P.TILED_SHAPES if s.name == "5x5 d(4,4) 96->96")))
    assert pn.load(k44, 3, 1, 2, 3, 0, 1) == 1 and pn.load(k44, 3, 1, 3, 2, 0, 1) == 0       # NC = 4 divides 4, NC = 8 does not
    ks2 = pn.key(P.geometry_desc(next(s for s in P.TILED_SHAPES if s.name == "3x3 s2 reflect 64->128")))
    assert pn.load(ks2, 2, 1, 0, 4, 0, 1) == 1 and pn.load(ks2, 2, 1, 1, 4, 0, 1) == 0       # NC > 1 at stride 2
    assert pn.load(ks2, 3, 1, 0, 4, 0, 1) == 0                           # three m-tiles of a 64-channel side
    assert pn.load(k55, 3, 1, 0, 4, 1, 2) == 0 and pn.load(k55, 1, 1, 0, 4, 1, 2) == 1       # LDS over 160 KB / 2
    assert pn.load(k55, 1, 1, 0, 4, 1, 4) == 0
    assert pn.load(k55, 1, 1, 0, 7, 1, 1) == 0                           # a tile one pixel wide


@pytest.mark.parametrize("change,code,message", [
    (dict(stride=2, dil=(2, 2)), P.EINVAL, "bad descriptor"),
    (dict(g_cs=100), P.EINVAL, "bad descriptor"),
    (dict(t_cin=64), P.EINVAL, "bad temporal taps"),
    (dict(k=(1, 33)), P.ENOSPC, "taps per row not supported")], ids=["stride-with-dilation", "g_cs%8", "t_cin%128", "33-taps-in-a-row"])
def test_descriptors_the_route_refuses(pinner, change, code, message):
    """sos_wgrad_describe returns the code (and message) the launch documents, and the launch agrees -- both host only."""
    import ctypes as C
    if "t_cin" in change:
        d = P.geometry_desc(P.Shape("probe", 32, 192, (3, 3), Hg=6, Wg=7, B=8, temporal=(4, 3, 64)))
    elif "g_cs" in change:
        d = _shape_desc(96, 96, (3, 3))
        d.g_cs = change["g_cs"]
    else:
        d = _shape_desc(96, 96, change.get("k", (3, 3)), dil=change.get("dil", (1, 1)), stride=change.get("stride", 1))
    rc, info = P.describe(pinner.h, d)
    msg = pinner.h.sos_last_error().decode()
    assert rc == code and info is None and message in msg, (rc, msg)
    assert pinner.h.sos_conv2d_wgrad(C.byref(d), None) == code


def _route(pn, d):
    rc, info = P.describe(pn.h, d)
    assert rc == 0, pn.h.sos_last_error().decode()
    return info.route


def test_route_boundaries(pinner, monkeypatch):
    pn = pinner
    one = dict(Hg=5, Wg=40, B=2)
    # the GEMM route: both sides of at least 128 channels
    assert _route(pn, _shape_desc(128, 128, **one)) == "gemm"
    assert _route(pn, _shape_desc(127, 128, **one)) == "tiled" == _route(pn, _shape_desc(128, 127, **one))
    monkeypatch.setenv("SOS_WGRAD_NO_GEMM", "1")
    assert _route(pn, _shape_desc(128, 128, **one)) == "tiled"
    monkeypatch.delenv("SOS_WGRAD_NO_GEMM")
    # the thin 1x1 route: one side of at most 16 channels and an instance for the other
    assert _route(pn, _shape_desc(48, 16, **one)) == "thin" == _route(pn, _shape_desc(16, 48, **one))
    assert _route(pn, _shape_desc(48, 17, **one)) == "tiled"
    assert _route(pn, _shape_desc(80, 14, **one)) == "tiled"             # m16 = 5: no instance
    flat = _shape_desc(48, 14, Hg=1, Wg=400, B=1)                        # arrives flat
    assert _route(pn, flat) == "thin"
    flat.g_cs = flat.g_off + 40                                          # g_off + 16 m16 > g_cs
    assert _route(pn, flat) == "tiled"
    # the thin taps route: 5 x 1, M in 49..64, N <= 16, whole 16-channel sub-images inside a pixel's channel run
    taps = lambda M=56, N=10, **kw: _shape_desc(M, N, (5, 1), **{**dict(Hg=5, Wg=33, pad=(2, 0)), **kw})
    for M in (49, 64):
        assert _route(pn, taps(M)) == "thin taps"
    for M in (48, 65):
        assert _route(pn, taps(M)) == "tiled"
    assert _route(pn, taps(N=16)) == "thin taps" and _route(pn, taps(N=17)) == "tiled"
    assert _route(pn, taps(Wg=32)) == "thin taps" and _route(pn, taps(Wg=31)) == "tiled"
    assert _route(pn, taps(stride=2, Hx=9, Wx=65)) == "tiled"
    assert _route(pn, taps(reflect=True, pad=(4, 0))) == "thin taps" and _route(pn, taps(reflect=True, pad=(5, 0))) == "tiled"
    short_g, short_x = taps(M=56), taps(N=10)
    short_g.g_off, short_g.g_cs = 0, 56                                  # the kernel fetches 64 channels of G ...
    short_x.x_off, short_x.x_cs = 0, 8                                   # ... and 16 of X, whatever M and N are
    assert _route(pn, short_g) == "tiled" == _route(pn, short_x)
    monkeypatch.setenv("SOS_WGRAD_NO_THIN", "1")
    assert _route(pn, taps()) == "tiled" == _route(pn, _shape_desc(48, 16, **one))
    monkeypatch.delenv("SOS_WGRAD_NO_THIN")
    # the 16x16x32 kernel: M and N in 33..48 with 25, 9 or 7 taps
    kind = lambda M, N, k: P.describe(pn.h, _shape_desc(M, N, k, Hg=11, Wg=13))[1].kind
    for k in ((5, 5), (3, 3), (7, 1)):
        assert kind(33, 48, k) == "wgrad16" == kind(48, 33, k)
        assert kind(32, 48, k) == "wgrad" == kind(48, 49, k)
    assert kind(48, 48, (5, 1)) == "wgrad" == kind(48, 48, (1, 1))
    monkeypatch.setenv("SOS_WGRAD_NO16_7", "1")
    assert kind(48, 48, (7, 1)) == "wgrad" and kind(48, 48, (3, 3)) == "wgrad16"


def test_forced_knobs_are_reported_or_fall_back_as_documented(pinner, monkeypatch):
    """SOS_WGRAD_MT / NTB / OCC / TILE bypass the table: describe reports the forced values where the plan is legal, and where it
    is not, the fallback wg_model_plan() documents: MT and NTB clamped to the shape's tiles, an NTB beyond 32 (tap, n-tile) pairs
    ignored, fewer workgroups per CU when the buffers do not fit, SOS_ENOSPC when SOS_WGRAD_TILE names a tile the shape cannot run."""
    pn = pinner
    d33 = P.geometry_desc(P.Shape("forced 3x3", 128, 128, (3, 3), Hg=19, Wg=27))
    d55 = P.geometry_desc(P.Shape("forced 5x5", 96, 96, (5, 5), (4, 4), Hg=19, Wg=27))
    free = P.describe(pn.h, d55)[1]
    monkeypatch.setenv("SOS_WGRAD_MT", "1")
    monkeypatch.setenv("SOS_WGRAD_NTB", "2")
    monkeypatch.setenv("SOS_WGRAD_OCC", "2")
    i = P.describe(pn.h, d33)[1]
    assert (i.mt, i.ntb, i.occ, i.instance) == (1, 2, 2, ("wgrad", 1, 2, 0))
    monkeypatch.setenv("SOS_WGRAD_NTB", "3")
    i = P.describe(pn.h, d33)[1]                                          # three n-tiles of the 3x3 patch do not fit half the LDS: one per CU
    assert (i.mt, i.ntb, i.occ, i.instance) == (1, 3, 1, ("wgrad", 1, 3, 0))
    i = P.describe(pn.h, d55)[1]                                          # 3 n-tiles x 25 taps > 32 pairs: NTB ignored
    assert (i.mt, i.ntb, i.occ, i.instance) == (1, 1, 2, ("wgrad", 1, 1, 0))
    monkeypatch.setenv("SOS_WGRAD_MT", "3")
    i = P.describe(pn.h, d55)[1]
    assert (i.mt, i.ntb, i.occ, i.instance) == (3, 1, 2, ("wgrad", 3, 1, 1))
    monkeypatch.setenv("SOS_WGRAD_OCC", "4")                              # four do not fit: as many workgroups per CU as the buffers allow
    i = P.describe(pn.h, d55)[1]
    assert (i.mt, i.ntb, i.instance) == (3, 1, ("wgrad", 3, 1, 1)) and 1 <= i.occ < 4 and i.lds <= 160 * 1024 // i.occ
    monkeypatch.setenv("SOS_WGRAD_NTB", "4")
    i = P.describe(pn.h, P.geometry_desc(P.Shape("forced 1x1", 40, 70, (1, 1), Hg=19, Wg=27)))[1]
    assert (i.mt, i.ntb) == (2, 3)                                       # clamped to the shape's 2 m-tiles and 3 n-tiles
    for name in ("SOS_WGRAD_MT", "SOS_WGRAD_NTB", "SOS_WGRAD_OCC"):
        monkeypatch.delenv(name)
    for tile in ("1,4,4,0", "1,4,4,1", "1,6,2,1", "1,2,6,0", "2,3,4,1", "4,4,2,1", "4,4,2,0"):
        monkeypatch.setenv("SOS_WGRAD_TILE", tile)
        i = P.describe(pn.h, d55)[1]
        assert (i.nc, i.lth, i.ltw, i.order) == tuple(int(v) for v in tile.split(",")), tile
    monkeypatch.setenv("SOS_WGRAD_TILE", "8,2,3,0")                       # 8 classes at dilation 4: no such plan
    assert P.describe(pn.h, d55)[0] == P.ENOSPC
    monkeypatch.setenv("SOS_WGRAD_TILE", "1,4,4,-1")                      # order left free: the cheaper of the two
    i = P.describe(pn.h, d55)[1]
    assert (i.nc, i.lth, i.ltw) == (1, 4, 4)
    monkeypatch.delenv("SOS_WGRAD_TILE")
    assert P.describe(pn.h, d55)[1] == free


def test_temporal_plans_keep_an_n_group_inside_one_frame(pinner, monkeypatch):
    """Found by tests/test_gpu_wgrad_plans.py: with temporal taps a workgroup reads its NTB n-tiles from ONE frame, and NTB = 3 (96
    columns) does not divide the 128-channel frames -- columns 128..191 of its second n-group were zeros.  wg_make_plan() now refuses
    n-groups that do not divide t_cin: such a line does not load, the forced knob falls back to two n-tiles, the cost model never
    picks it, and no line of the shipped table is affected (it still loads completely)."""
    from sos_amd import engine
    pn = pinner
    s = next(s for s in P.TILED_SHAPES if s.temporal)
    d = P.geometry_desc(s)
    key = pn.key(d)
    assert key[10] == s.temporal[1]
    assert pn.load(key, 1, 2, 0, 5, 0, 1) == 1 and pn.load(key, 1, 3, 0, 5, 0, 1) == 0 and pn.load(key, 1, 1, 0, 5, 0, 1) == 1
    assert {p[1] for p in pn.offered(d)} == {1, 2}
    monkeypatch.setenv("SOS_WGRAD_NTB", "3")
    assert P.describe(pn.h, d)[1].ntb == 2
    monkeypatch.delenv("SOS_WGRAD_NTB")
    for kt, tcin, M in ((3, 128, 96), (5, 128, 64), (3, 256, 128), (5, 384, 32)):       # the cost model's own picks
        probe = P.geometry_desc(P.Shape("temporal probe", M, kt * tcin, (3, 3), Hg=11, Wg=13, B=8, temporal=(4, kt, tcin)))
        info = P.describe(pn.h, probe)[1]
        assert tcin % (32 * info.ntb) == 0, info
    lines = [ln.split() for ln in open(engine.SHIPPED_WGRAD_TABLE).read().splitlines()[1:] if ln.strip()]
    for v in lines:
        taps, N, ntb = int(v[10]), int(v[8]), int(v[13])
        assert taps <= 1 or (N // taps) % (32 * ntb) == 0, v
    assert pn.h.sos_wgrad_tune_load(engine.SHIPPED_WGRAD_TABLE.encode()) == len(lines)
