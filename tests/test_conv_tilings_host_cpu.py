"""Which tilings the forward convolution OFFERS for the shapes of tests/test_gpu_conv_tilings.py, asked of the library itself
(sos_conv2d_tune_load accepts an entry iff enumerate_cfgs() offers it; host only, no GPU): together the shapes reach every compiled
kernel instance and every tile-geometry kind, the instances that are compiled but never offered stay unoffered, and what
enumerate_cfgs() must refuse is refused."""
import os
import re

import pytest

import conv_pin as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if P.forcing_switch():
    pytest.skip(P.forcing_switch(), allow_module_level=True)

KINDS = {"pow2", "row", "tall", "tw8", "npot", "npot-odd", "classes", "classes-npot", "classes3", "slots384", "slots3xx"}


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def pinner(request):
    """One Pinner per build of the library (bfloat16 / IEEE half storage)."""
    import sos_amd
    sos_amd.set_precision(request.param)
    try:
        p = P.Pinner()
        yield p
        p.close()
    finally:
        sos_amd.set_precision("bf16")


def compiled_instances():
    """conv_instances of csrc/conv.hip, its macros expanded: {(row16, nt, ks, nbuf, w3, slots, inbn)}."""
    src = open(os.path.join(ROOT, "listening-to-sound-of-silence-for-speech-denoising_amd", "csrc", "conv.hip")).read()
    body = src[src.index("static const ConvInstance conv_instances[] = {"):]
    body = body[body.index("{") + 1:body.index("};")]
    body = re.sub(r"//[^\n]*", "", body)
    out = set()
    for nt in re.findall(r"SOS_K32_DOUBLE\((\d)\)", body):
        out |= {(False, int(nt), ks, 2, False, 256, False) for ks in (1, 2, 3, 4, 5, 6, 8)}
    for nt in re.findall(r"SOS_K32_SINGLE\((\d)\)", body):
        out |= {(False, int(nt), ks, 1, False, 256, False) for ks in (1, 2, 3, 4)}
    for nt, ks, sb, inbn, pt, w3 in re.findall(r"SOS_K32\((\d), (\d), (\w+), (\w+), (\d), (\w+)\)", body):
        out.add((False, int(nt), int(ks), 1 if sb == "true" else 2, w3 == "true", 128 * int(pt), inbn == "true"))
    for nt, ks in re.findall(r"SOS_K16\((\d), (\d)\)", body):
        out |= {(True, int(nt), int(ks), nbuf, False, 256, False) for nbuf in (2, 1)}
    return out


def test_expected_instances_are_the_compiled_ones():
    """conv_pin.INSTANCES is conv_instances without the two fused-input-BatchNorm entries (those are reached by
    test_gpu_conv_tilings.py::test_fused_input_batchnorm): a new instance must be added there, with a shape that reaches it."""
    built = compiled_instances()
    assert {i[:6] for i in built if not i[6]} == set(P.INSTANCES) and len(P.INSTANCES) == len(set(P.INSTANCES))
    assert {i[:6] for i in built if i[6]} == {(False, 3, 2, 2, False, 256), (False, 3, 3, 2, False, 256)}
    assert set(P.DEAD_INSTANCES) <= set(P.INSTANCES)


def test_shapes_reach_every_instance_and_every_geometry_kind(pinner):
    """Every ks code of the file format is loaded for every shape (no code is left out on the word of a rule copied into
    conv_pin.candidates(): the pruned list the GPU tests use must get the same verdicts), and tiles below 160 pixels -- the one thing
    both lists leave out -- are asked of the library with every code as well."""
    reached, kinds = {}, {}
    for s in P.ALL_SHAPES:
        for mode in ("bf16", "bf16x3"):           # (the two shape keys of a 16-bit launch: one channel segment, three)
            d = P.geometry_desc(s, mode)
            tilings = P.offered(pinner, d, every_code=True)
            assert tilings, f"{s.name}: nothing offered"
            assert tilings == P.offered(pinner, d), f"{s.name} {mode}: candidates() prunes a ks code the library offers"
            key = P.shape_key(d)
            for small in ((1, 8, 8), (1, 12, 13), (1, 3, 53), (min(2, s.dil[1]), 6, 13)):
                assert not [ks for ks in P.KS_CODES if pinner.load(key, *small, ks)], f"{s.name}: a tile of {small} is offered"
            for (NC, TH, TW, ks) in tilings:
                reached.setdefault(P.decode(ks, d), s.name)
            for (NC, TH, TW, ks, kind) in P.select(tilings):
                kinds.setdefault(kind, s.name)
    for inst, why in P.DEAD_INSTANCES.items():
        assert inst not in reached, f"{inst} is offered now ({reached.get(inst)}): add coverage for it ({why})"
    missing = [i for i in P.INSTANCES if i not in reached and i not in P.DEAD_INSTANCES]
    assert not missing, f"instances no shape reaches: {missing}"
    assert set(kinds) == KINDS, (sorted(KINDS - set(kinds)), sorted(set(kinds) - KINDS))


def test_no_shipped_tiling_exceeds_the_fused_batchnorm_staging(pinner):
    """plan() refuses a descriptor with in_scale on tilings whose patch needs more than 64 staging instructions.  No entry of the
    shipped table that names one of the two fused-BatchNorm instances (three n-tiles, 2 or 3 k-steps, two slabs; a three-per-CU
    entry runs as that twin) may be such a tiling: with in_scale set, each of those shapes still resolves to ITS table entry."""
    from sos_amd import _lib as L
    n = 0
    for ln in open(__import__("sos_amd").engine.SHIPPED_TUNE_TABLE).read().splitlines()[1:]:
        v = [int(x) for x in ln.split()]
        if len(v) != 23:
            continue
        k, ks = v[:19], v[22]
        if k[5] != 1 or k[14] != L.DT_BF16 or k[15] != 1 or k[17] or ks <= 0:
            continue
        d = L.ConvDesc()
        (d.B, d.H, d.W, d.Wl, d.cin, d.in_nseg, d.cout_pad, d.kh, d.kw, d.stride, d.dil_h, d.dil_w, d.Ho, d.Wo, d.out_dtype) = k[:15]
        d.out_sc, d.pad_mode, d.cout, d.cout_store = 1, k[16], k[18], k[6]
        d.in_cs = d.in_seg_stride = d.cin
        d.out_sw, d.out_sh, d.out_sb = d.cout_pad, d.Wo * d.cout_pad, d.Ho * d.Wo * d.cout_pad
        d.pad_top, d.pad_left = (d.kh - 1) // 2 * d.dil_h, (d.kw - 1) // 2 * d.dil_w
        inst = P.decode(ks, d)
        if inst[:4] not in ((False, 3, 2, 2), (False, 3, 3, 2)) or inst[5] != 256:
            continue
        assert pinner.load(tuple(k), v[19], P.tdim(v[20]), P.tdim(v[21]), ks) == 1
        d.in_scale = d.in_shift = 1
        tiles, listed = pinner.resolved(d)
        assert tiles == P.tile_count(d, v[19], P.tdim(v[20]), P.tdim(v[21])) and not listed, (ln, tiles, listed)
        n += 1
    assert n >= 20, n


def test_pruned_candidates_are_refused_by_the_library(pinner):
    """conv_pin.candidates() leaves out codes and tile sizes no rule of enumerate_cfgs() produces: the library says 0 to them."""
    by_name = {s.name: s for s in P.ALL_SHAPES}
    d = P.geometry_desc(by_name["5x5d(2,3) 96->29"], "bf16")        # one n-tile, cin / 16 = 6
    key = P.shape_key(d)
    assert pinner.load(key, 1, 16, 16, 6) == 1
    for c in [(1, 16, 16, 4), (1, 16, 16, 5), (1, 16, 16, 8),       # k-steps that do not divide cin / 16
              (1, 16, 16, 0), (1, 16, 16, -1),                      # the 16-row kernel: cin is neither 16 nor 48
              (1, 16, 16, 202), (1, 16, 24, 302), (1, 16, 16, 2002),  # three per CU / 384 slots / two n-blocks: not with one n-tile
              (1, 8, 8, 6), (1, 12, 13, 6),                         # fewer than 160 pixels
              (1, 16, 16, 402), (1, 16, 16, 7)]:                    # no such code
        assert pinner.load(key, *c) == 0, c


def test_load_verdicts(pinner):
    by_name = {s.name: s for s in P.ALL_SHAPES}
    d = P.geometry_desc(by_name["5x5d(2,3) 96->88 f"], "bf16")      # dil_w = 3, three n-tiles, cin / 16 = 6
    key = P.shape_key(d)
    assert pinner.load(key, 2, 8, 16, 3) == 1 and pinner.load(key, 3, 7, 12, 3) == 1
    assert pinner.load(key, 4, 8, 8, 3) == 0                        # NC > dil_w
    assert pinner.load(key, 6, 7, 6, 3) == 0
    assert pinner.load(key, 1, 16, 16, 4) == 0                      # ks does not divide cin / 16
    assert pinner.load(key, 1, 16, 32, 3) == 0                      # 512 pixels in 256 slots
    assert pinner.load(key, 2, 13, 12, 302) == 1                    # 312 of 384 slots
    assert pinner.load(key, 2, 16, 16, 302) == 0                    # 512 pixels in 384 slots
    assert pinner.load(key, 2, 13, 16, 302) == 0                    # 416
    d2 = P.geometry_desc(by_name["5x5s2r 64->60"], "bf16")
    k2 = P.shape_key(d2)
    assert pinner.load(k2, 1, 16, 16, 2) == 1
    assert pinner.load(k2, 2, 8, 16, 2) == 0                        # NC > 1 with stride 2


def test_pin_takes_effect_or_fails(pinner):
    """pin() = load + the resolved tile count: the pinned tiling is the one the next launch of the descriptor uses; a tiling that
    is not offered, or that plan() refuses for the descriptor, is an assertion and not a silent run of the default tiling."""
    by_name = {s.name: s for s in P.ALL_SHAPES}
    s = by_name["5x5d(2,3) 96->88 f"]
    d = P.geometry_desc(s, "bf16")
    assert pinner.pin(d, 3, 7, 12, 3) == 2 * 2 * 2 * 1 * 1          # B x dil_h x ceil(13 / 7) x ceil(3 / 3) x ceil(12 / 12)
    assert pinner.pin(d, 1, 16, 16, 2) == 2 * 2 * 1 * 3 * 1
    with pytest.raises(AssertionError):
        pinner.pin(d, 4, 8, 8, 3)
    # 384-slot tiles do not run ragged batches: the entry loads for the SHAPE, the ragged descriptor resolves to another tiling
    assert pinner.pin(d, 2, 13, 12, 302) == 2 * 2 * 1 * 2 * 1
    d.wl_tab, d.wo_tab = 1, 1
    with pytest.raises(AssertionError, match="cfg 0/"):             # (it took the cost model's first candidate)
        pinner.pin(d, 2, 13, 12, 302)
    # three per CU with accumulation: take_entry() runs the plain twin -- same tile, same count, nothing listed
    d = P.geometry_desc(s, "bf16")
    d.accumulate = 1
    with pytest.raises(AssertionError, match="plain twin"):
        pinner.pin(d, 1, 16, 16, 202)
    assert pinner.resolved(d) == (12, "") and pinner.pin(d, 1, 16, 16, 2) == 12
    # fused input BatchNorm: its staging moves at most 64 instructions (768 patch pixels at two k-steps), a 1 x 256 tile has 5 x 260
    d = P.geometry_desc(s, "bf16")
    d.in_scale = d.in_shift = 1
    assert pinner.pin(d, 1, 16, 16, 2) == 12 and pinner.pin(d, 2, 8, 16, 3) == 16
    with pytest.raises(AssertionError, match="cfg 0/"):
        pinner.pin(d, 1, 1, 256, 2)
    with pytest.raises(AssertionError, match="cfg 0/"):
        pinner.pin(d, 1, 16, 16, 6)


def test_no_test_shape_is_in_the_shipped_table():
    descs = [P.geometry_desc(s, mode, out) for s in P.ALL_SHAPES for mode in ("bf16", "bf16x3") for out in ("16", "f32", "f32s")]
    P.assert_not_shipped(descs)
