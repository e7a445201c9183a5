"""train_ops.phase_taps, the one statement of "the data gradient of a stride-s conv is s*s stride-1 convs over dy, one per input
phase", and its three callers (the U-Net's stride-2 blocks, its transposed convs, the video branch).  Host only: no device.

* the rule against float64 autograd: dx of conv2d rebuilt from dy by the correlations the rule describes;
* the down and the up plan against the literal tap tables they carried before the rule existed, restated here;
* the number of pack_weight calls per plan builder (engine.PackRecorder hands packed tensors out by call index)."""
import pytest
import torch
import torch.nn.functional as F

# every (k, s, pad, image) of the grid at which conv2d is defined (the padded image holds the kernel): 38 cases; k 3, s 3, pad 1 --
# the video branch's stride-3 blocks, whose last phase has a NEGATIVE left pad -- is among them
GRID = [(k, s, pad, hw) for k in (1, 3, 5, 7) for s in (2, 3) for pad in range(k // 2 + 1) for hw in ((7, 9), (8, 5))
        if min(hw) + 2 * pad >= k]


def _place(t, left, length, dim):
    """`t` shifted right by `left` cells (left by -left: a crop) along `dim` inside `length` zeros."""
    out_shape = list(t.shape)
    out_shape[dim] = length
    out = t.new_zeros(out_shape)
    lo, hi = max(left, 0), min(left + t.shape[dim], length)
    if hi > lo:
        out.narrow(dim, lo, hi - lo).copy_(t.narrow(dim, lo - left, hi - lo))
    return out


def test_grid_holds_the_video_case():
    assert (3, 3, 1, (7, 9)) in GRID and (3, 3, 1, (8, 5)) in GRID and len(GRID) == 38


@pytest.mark.parametrize("k,s,pad,hw", GRID, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rule_against_float64_autograd(k, s, pad, hw):
    """Bound 1e-12: a sum of at most 49 * 3 products of N(0, 1) values in float64 (eps 2.2e-16) errs below 1e-13; one decade
    above that.  Not taken from the code under test."""
    from sos_amd.train_ops import phase_taps
    g = torch.Generator().manual_seed(1000 * k + 100 * s + 10 * pad + hw[0])
    x = torch.randn((2, 2) + hw, dtype=torch.float64, generator=g).requires_grad_()
    w = torch.randn((3, 2, k, k), dtype=torch.float64, generator=g)
    y = F.conv2d(x, w, stride=s, padding=pad)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(dy)
    H, W = hw
    dx = torch.zeros_like(x)
    for rh in range(s):
        th, ph = phase_taps(k, s, pad, rh)
        for rw in range(s):
            tw, pw = phase_taps(k, s, pad, rw)
            Hp, Wp = (H - rh + s - 1) // s, (W - rw + s - 1) // s
            if not th or not tw or Hp < 1 or Wp < 1:
                continue
            sub = w[:, :, th][:, :, :, tw].transpose(0, 1)                                   # (I, O, Mh, Mw), packed order
            dyp = _place(_place(dy, ph, Hp + len(th) - 1, 2), pw, Wp + len(tw) - 1, 3)       # a negative left pad crops dy
            dx[:, :, rh::s, rw::s] = F.conv2d(dyp, sub)
    err = float((dx - x.grad).abs().max())
    print(f"[phase-rule] k {k} s {s} pad {pad} {H}x{W}: max abs err {err:.2e}")
    assert err <= 1e-12


def test_negative_left_pad():
    from sos_amd.train_ops import phase_taps
    assert phase_taps(3, 3, 1, 2) == ([0], -1)
    assert phase_taps(3, 3, 1, 0) == ([1], 0) and phase_taps(3, 3, 1, 1) == ([2], 0)
    assert phase_taps(1, 2, 0, 1) == ([], -1)              # no tap reaches this phase: skipped by the callers


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "bf16x3"])
@pytest.mark.parametrize("k,in_perm", [(3, None), (5, None), (7, None), (3, [2, 0, 1, 3, 5, 4])])
def test_down_plan_against_its_literal_taps(k, in_perm, x3):
    from sos_amd import engine as E, train_ops as TO
    from sos_amd.denoiser.networks import DownConvBlock
    torch.manual_seed(k)
    blk = DownConvBlock(6, 5, k, 2)
    lp = TO.down_train_plan(blk, x3, in_perm)
    w = blk.block[1].weight.detach().float()
    if in_perm is not None:
        w = w[:, in_perm]
    assert list(lp["wd_phases"]) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for ph in (0, 1):
        for pw in (0, 1):
            Mh, Mw = (k + 1 - ph) // 2, (k + 1 - pw) // 2
            a = [ph + 2 * (Mh - 1 - t) for t in range(Mh)]
            b = [pw + 2 * (Mw - 1 - t) for t in range(Mw)]
            want = E.pack_weight(w[:, :, a][:, :, :, b].transpose(0, 1).contiguous(), 16, x3)
            got = lp["wd_phases"][(ph, pw)]
            assert torch.equal(got[0], want)
            assert got[1:] == (Mh, Mw, Mh - 1, Mw - 1)      # pad 0 on the reflect-padded domain: the full left pad


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "bf16x3"])
def test_up_plan_against_its_literal_taps(x3):
    from sos_amd import engine as E, train_ops as TO
    from sos_amd.denoiser.networks import UpConvBlock
    torch.manual_seed(7)
    blk = UpConvBlock(6, 5, 3, 2)
    lp = TO.up_train_plan(blk, x3)
    w = blk.block[0].weight.detach().float()                # (Cin, Cout, 3, 3)
    taps = {0: [1], 1: [2, 0]}
    assert list(lp["phases"]) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for ph in (0, 1):
        for pw in (0, 1):
            want = E.pack_weight(w[:, :, taps[ph]][:, :, :, taps[pw]].permute(1, 0, 2, 3).contiguous(), 16, x3)
            got = lp["phases"][(ph, pw)]
            assert torch.equal(got[0], want)
            assert got[1:] == (1 + ph, 1 + pw, 0, 0)


def _count_packs(monkeypatch, build):
    from sos_amd import engine as E
    calls, real = [], E.pack_weight

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(E, "pack_weight", counting)
    plan = build()
    monkeypatch.setattr(E, "pack_weight", real)
    return len(calls), plan


def test_pack_weight_calls_per_builder(monkeypatch):
    """The counts of the code before the rule: the forward weight, then s*s phases less the ones without taps (none at these
    kernels), then -- the up block -- its data-gradient weight."""
    from sos_amd import common_nets as CN, train_ops as TO
    from sos_amd.denoiser.networks import DownConvBlock, UpConvBlock
    torch.manual_seed(3)
    n, _ = _count_packs(monkeypatch, lambda: TO.down_train_plan(DownConvBlock(6, 5, 5, 2), False))
    assert n == 1 + 4
    n, _ = _count_packs(monkeypatch, lambda: TO.up_train_plan(UpConvBlock(6, 5, 3, 2), False))
    assert n == 4 + 1
    stack = torch.nn.Sequential(CN.Conv3dBlock(3, 8, (3, 3, 3), (1, 2, 2)), CN.Conv3dBlock(8, 8, (3, 3, 3), (1, 3, 3)))
    n, plan = _count_packs(monkeypatch, lambda: TO.video_train_plan(stack, False))
    assert n == (1 + 4) + (1 + 9)
    assert len(plan[0]["wd_phases"]) == 4 and len(plan[1]["wd_phases"]) == 9
    assert plan[1]["wd_phases"][(2, 2)][1:] == (1, 1, -1, -1)
    # a block with the temporal taps inside the kernels (whole 128-channel frames, stride 2)
    native = torch.nn.Sequential(CN.Conv3dBlock(128, 16, (3, 3, 3), (1, 2, 2)))
    n, plan = _count_packs(monkeypatch, lambda: TO.video_train_plan(native, False))
    assert plan[0]["native"] and n == 1 + 4
