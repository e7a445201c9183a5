"""Float64 reference of the BatchNorm + activation kernels of csrc/bn.hip, at the kernels' boundary (tests/test_gpu_batchnorm.py),
pinned against torch.nn.BatchNorm2d / BatchNorm3d in tests/test_bn_reference.py.

Tensors are NHWC rows [npix, C] (channels last, one row per pixel) of the values the buffers actually hold, on any device;
everything is computed in float64.  The conventions are the kernels' (bn.hip, header of the backward section):
  forward : mean, biased var; invstd = 1 / sqrt(var + eps); scale = gamma * invstd, shift = beta - mean * scale;
            running_mean / running_var with momentum and the UNBIASED variance; y = act(x * scale + shift)
  backward: z = x * scale + shift (from the f32 scale / shift the forward kept), dz = dy * act'(z),
            xhat = (x - mean) * invstd;  S1 = sum dz, S2 = sum dz * xhat, S3 = sum_{z < 0} dy * z;
            dgamma = S2, dbeta = S1, dslope = sum_c S3 (each times out_scale);  dx = a dz + b xhat + c with
            a = gamma * invstd, b = -a S2 / N, c = -a S1 / N.  mean = None: bias + activation only, xhat = x, dx = dz.
ReLU passes the gradient where z > 0; PReLU uses 1 where z >= 0 and the slope elsewhere."""
import torch

NONE, RELU, PRELU, SIGMOID = 0, 1, 2, 3          # SOS_ACT_* of include/sos_hip.h
EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # the f32 eps / momentum the kernels are handed
MOMENTUM = float(torch.tensor(0.1, dtype=torch.float32))


def _f64(t):
    return None if t is None else torch.as_tensor(t).double()


def act(z, kind, slope=0.0):
    if kind == RELU:
        return z.clamp_min(0.0)
    if kind == PRELU:
        return torch.where(z >= 0, z, slope * z)
    if kind == SIGMOID:
        return torch.sigmoid(z)
    assert kind == NONE, kind
    return z


def act_grad(z, kind, slope=0.0):
    if kind == RELU:
        return (z > 0).double()
    if kind == PRELU:
        return torch.where(z >= 0, torch.ones_like(z), torch.full_like(z, slope))
    if kind == SIGMOID:
        s = torch.sigmoid(z)
        return s * (1.0 - s)
    assert kind == NONE, kind
    return torch.ones_like(z)


def stats(x, gamma=None, beta=None, eps=EPS):
    """Batch statistics of x [npix, C] and the finalize's coefficients: dict of float64 [C] mean, var (biased), invstd,
    scale, shift."""
    x = _f64(x)
    mean = x.mean(0)
    var = (x - mean).square().mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones_like(mean) if gamma is None else _f64(gamma).to(x.device)
    b = torch.zeros_like(mean) if beta is None else _f64(beta).to(x.device)
    scale = g * invstd
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=b - mean * scale, count=x.shape[0])


class Running:
    """running_mean / running_var / num_batches_tracked of one layer (torch's initial 0 / 1 / 0), float64."""

    def __init__(self, C, device="cpu", momentum=MOMENTUM):
        self.mean = torch.zeros(C, dtype=torch.float64, device=device)
        self.var = torch.ones(C, dtype=torch.float64, device=device)
        self.num_batches_tracked = 0
        self.momentum = momentum

    def step(self, st):
        """One training step with the statistics `st` of stats()."""
        n, m = st["count"], self.momentum
        self.mean = (1.0 - m) * self.mean + m * st["mean"]
        self.var = (1.0 - m) * self.var + m * st["var"] * n / max(n - 1, 1)
        self.num_batches_tracked += 1
        return self


def apply(x, scale, shift, kind, slope=0.0):
    """y = act(x * scale + shift), float64 [npix, C]."""
    x = _f64(x)
    return act(x * _f64(scale).to(x.device) + _f64(shift).to(x.device), kind, slope)


def forward(x, gamma=None, beta=None, kind=RELU, slope=0.0, eps=EPS):
    """Training-mode BatchNorm + activation: (y, stats)."""
    st = stats(x, gamma, beta, eps)
    return apply(x, st["scale"], st["shift"], kind, slope), st


def backward(x, dy, scale, shift, mean, invstd, gamma, kind, slope=0.0, out_scale=1.0):
    """The closed-form backward of the kernels (module docstring).  scale / shift / mean / invstd are the forward's f32
    values (z in float64 from them: the activation mask is the kernel's); mean = invstd = None: the bias + activation mode.
    Returns dict of float64 S1, S2, S3, dgamma, dbeta [C], dslope (scalar), dx [npix, C], the coefficients a, b, c [C] and
    the per-channel sums of |terms| of S1 / S2 / S3 (for tolerances of reductions: t1, t2, t3)."""
    x, dy = _f64(x), _f64(dy).to(x.device)
    dev = x.device
    z = x * _f64(scale).to(dev) + _f64(shift).to(dev)
    dz = dy * act_grad(z, kind, slope)
    xhat = x if mean is None else (x - _f64(mean).to(dev)) * _f64(invstd).to(dev)
    neg = z < 0
    s3_terms = torch.where(neg, dy * z, torch.zeros_like(z))
    S1, S2, S3 = dz.sum(0), (dz * xhat).sum(0), s3_terms.sum(0)
    n = x.shape[0]
    if mean is None:
        a = torch.ones_like(S1)
        b = torch.zeros_like(S1)
        c = torch.zeros_like(S1)
    else:
        a = (torch.ones_like(S1) if gamma is None else _f64(gamma).to(dev)) * _f64(invstd).to(dev)
        b = -a * S2 / n
        c = -a * S1 / n
    dx = dz if mean is None else a * dz + b * xhat + c
    return dict(S1=S1, S2=S2, S3=S3, dgamma=S2 * out_scale, dbeta=S1 * out_scale, dslope=S3.sum() * out_scale, dx=dx,
                a=a, b=b, c=c, t1=dz.abs().sum(0), t2=(dz * xhat).abs().sum(0), t3=s3_terms.abs().sum(0),
                dx_terms=(a * dz).abs() + (b * xhat).abs() + c.abs())
