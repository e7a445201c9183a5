"""CPU pin of tests/bn_reference.py (the float64 reference of the BatchNorm kernels' GPU tests): the same values as
torch.nn.BatchNorm2d / BatchNorm3d in train mode followed by ReLU / PReLU / Sigmoid, all in float64 autograd -- output, running
statistics after one and two steps, num_batches_tracked, dx, dgamma, dbeta, the PReLU slope gradient -- and the bias +
activation mode (mean = None) against autograd of act(x + bias)."""
import pytest
import torch

import bn_reference as R

TOL = 1e-12


def _close(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    err = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)
    assert err < TOL, (what, err)


def _rows(x):
    """[B, C, *spatial] -> NHWC rows [npix, C]."""
    return x.movedim(1, -1).reshape(-1, x.shape[1])


def _module_act(kind, slope):
    if kind == R.RELU:
        return torch.nn.ReLU()
    if kind == R.PRELU:
        m = torch.nn.PReLU(1, init=slope).double()
        return m
    if kind == R.SIGMOID:
        return torch.nn.Sigmoid()
    return torch.nn.Identity()


@pytest.mark.parametrize("dims", [2, 3], ids=["BatchNorm2d", "BatchNorm3d"])
@pytest.mark.parametrize("kind", [R.NONE, R.RELU, R.PRELU, R.SIGMOID], ids=["none", "relu", "prelu", "sigmoid"])
def test_reference_matches_torch_batchnorm(dims, kind):
    g = torch.Generator().manual_seed(17 + 4 * dims + kind)
    C = 5
    shape = (3, C, 4, 7) if dims == 2 else (2, C, 3, 4, 5)
    bn = (torch.nn.BatchNorm2d if dims == 2 else torch.nn.BatchNorm3d)(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64))
        bn.bias.copy_(0.2 * torch.randn(C, generator=g, dtype=torch.float64))
    slope = 0.25
    am = _module_act(kind, slope)
    run = R.Running(C, momentum=bn.momentum)      # (the kernels get the f32 value of 0.1: R.MOMENTUM)
    for step in range(2):
        # per-channel offsets: the variance is not the sum of squares
        x = torch.randn(shape, generator=g, dtype=torch.float64) + torch.arange(C, dtype=torch.float64).view(1, C, *([1] * dims))
        x.requires_grad_(True)
        dy = torch.randn(shape, generator=g, dtype=torch.float64)
        for p in list(bn.parameters()) + list(am.parameters()):
            p.grad = None
        y = am(bn(x))
        (y * dy).sum().backward()
        yr, st = R.forward(_rows(x.detach()), bn.weight.detach(), bn.bias.detach(), kind, slope)
        _close(yr, _rows(y.detach()), "y")
        run.step(st)
        _close(run.mean, bn.running_mean, f"running_mean step {step + 1}")
        _close(run.var, bn.running_var, f"running_var step {step + 1}")
        assert run.num_batches_tracked == int(bn.num_batches_tracked) == step + 1
        b = R.backward(_rows(x.detach()), _rows(dy), st["scale"], st["shift"], st["mean"], st["invstd"], bn.weight.detach(), kind,
                       slope)
        _close(b["dx"], _rows(x.grad), "dx")
        _close(b["dgamma"], bn.weight.grad, "dgamma")
        _close(b["dbeta"], bn.bias.grad, "dbeta")
        if kind == R.PRELU:
            _close(b["dslope"], am.weight.grad.sum(), "dslope")


def test_reference_out_scale_scales_the_parameter_gradients_only():
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(40, 3, generator=g, dtype=torch.float64), torch.randn(40, 3, generator=g, dtype=torch.float64)
    st = R.stats(x)
    one = R.backward(x, dy, st["scale"], st["shift"], st["mean"], st["invstd"], None, R.PRELU, 0.25)
    sc = R.backward(x, dy, st["scale"], st["shift"], st["mean"], st["invstd"], None, R.PRELU, 0.25, out_scale=0.125)
    for k in ("dgamma", "dbeta", "dslope"):
        _close(sc[k], one[k] * 0.125, k)
    _close(sc["dx"], one["dx"], "dx")


@pytest.mark.parametrize("kind", [R.NONE, R.RELU, R.PRELU, R.SIGMOID], ids=["none", "relu", "prelu", "sigmoid"])
def test_reference_bias_activation_mode(kind):
    """mean = invstd = None (sos_bn_bwd without BatchNorm): dx = d(pre-activation), dbeta = dbias, dgamma = sum dz * x."""
    g = torch.Generator().manual_seed(11 + kind)
    C, slope = 6, 0.25
    x = torch.randn(50, C, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(50, C, generator=g, dtype=torch.float64)
    am = _module_act(kind, slope)
    pre = x + bias
    pre.retain_grad()
    y = am(pre)
    (y * dy).sum().backward()
    b = R.backward(x.detach(), dy, torch.ones(C, dtype=torch.float64), bias.detach(), None, None, None, kind, slope)
    _close(b["dx"], x.grad, "dx")
    _close(b["dbeta"], bias.grad, "dbias")
    _close(b["dgamma"], (pre.grad * x.detach()).sum(0), "S2 (x for xhat)")
    if kind == R.PRELU:
        _close(b["dslope"], am.weight.grad.sum(), "dslope")
