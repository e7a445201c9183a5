"""The recurrent kernels of lstm.hip (sos_lstm_bidir_fwd / sos_lstm_bidir_bwd) and the whole BiLSTM training layer
(train_ops.lstm_*) against the float64 reference of tests/lstm_reference.py, on every compiled path of the forward:

  - resident W_hh (16-bit modes, H = 100: lstm_fwd_kernel<false, 4, 4>; H = 200: <false, 4, 7>),
  - W_hh streamed from L2 (16-bit modes, every other H, and H = 100 / 200 under SOS_LSTM_STREAM_W=1: <false, 0, 8>;
    an odd tile count per wave runs the wrap-around fix-up of the one-tile-ahead prefetch),
  - the three-pass bf16x3 kernel (<true>),
  - 16-byte flushes of h (H % 8 == 0) and element stores (H % 8 != 0), more than one 16-clip group, partial groups,
    ragged batches (per-clip lengths).

Tolerances (relative to the largest |value| of the exact reference): bf16x3 a flat bound; bf16 / fp16 the kernel's deviation
from the exact reference must lie within MODEL_FACTOR x the deviation of the storage-rounding model (the reference with round
trips where the kernels store in 16 bits) + FLOOR, and under an absolute per-mode CEIL that does not follow the model."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lstm_reference import bilstm, to_kernel_order, to_torch_order
from util import hashed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SENT = 7.0                 # sentinel of the 16-bit buffers: exact in bf16 and fp16, outside tanh's range
GUARD_F32 = 4096           # sentinel floats after the f32 buffers (saved gates / cell state / dgates)
# 16-bit modes: kernel deviation <= MODEL_FACTOR x model deviation + FLOOR (as tests/test_gpu_pipeline.py).  Observed on MI355X,
# kernel / model: h 1.00 in every case (the forward rounds exactly where the model does), dgates 0.93-1.05, parameter gradients
# and dfeat of the training layer 0.85-1.20.  FLOOR covers cases whose deviations are at f32's level (observed down to 1.9e-7).
MODEL_FACTOR = 2.0
FLOOR = 1e-6
# bf16x3: flat bounds relative to max |h| / max |dgates| / max |gradient| of the exact reference.  Observed on MI355X (worst case
# over the lists below): h 7.4e-6, dgates 3.2e-6, training-layer gradients and dfeat 7.7e-6.
TOL_X3 = dict(h=1e-5, dgates=6e-6, grad=1.5e-5)
# absolute ceilings of the 16-bit modes, independent of the model (same scales).  Observed on MI355X (worst case):
# bf16 h 4.0e-3, dgates 1.4e-3, gradients 3.6e-3; fp16 h 5.1e-4, dgates 1.6e-4, gradients 4.9e-4.
CEIL = {"bf16": dict(h=6e-3, dgates=2.5e-3, grad=5.5e-3), "fp16": dict(h=8e-4, dgates=2.5e-4, grad=7.5e-4)}


@pytest.fixture(params=["bf16", "fp16", "bf16x3"])
def mode(request):
    """The kernels' storage modes: bfloat16 and IEEE half (the two library builds) and the three-pass split."""
    import sos_amd
    sos_amd.set_precision(request.param)
    try:
        yield request.param
    finally:
        sos_amd.set_precision("bf16")


def _storage(mode):
    return {"bf16": torch.bfloat16, "fp16": torch.float16}.get(mode)


def _ceil16(b):
    return (b + 15) // 16 * 16


def _rel(a, b, scale):
    return float((a.double() - b.double()).abs().max()) / scale


def _check(mode, what, err_k, err_m):
    """bf16x3: err_k < TOL_X3[what]; 16-bit: err_k <= MODEL_FACTOR * err_m + FLOOR and err_k < CEIL[mode][what]."""
    print(f"[lstm] {mode} {what}: kernel {err_k:.2e}" + ("" if err_m is None else f" model {err_m:.2e}"))
    if mode == "bf16x3":
        assert err_k < TOL_X3[what], (what, err_k)
    else:
        assert err_k <= MODEL_FACTOR * err_m + FLOOR, (what, err_k, err_m)
        assert err_k < CEIL[mode][what], (what, err_k)


def _whh(H, seed):
    """W_hh [2][4H][H] of both directions, U(-1.5, 1.5) / sqrt(H): a recurrent term of O(1) next to the projection."""
    return torch.from_numpy(hashed(seed, (2, 4 * H, H), 1.5 / np.sqrt(H)).astype(np.float32))


def _xproj(B, T, H, seed):
    """Gate pre-activations U(-3, 3): saturated on some elements, not on others."""
    x = hashed(seed, (B, T, 2, 4 * H), 3.0).astype(np.float32)
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def _ref_h(H, B, T, wseed, xseed, lengths=None, dtype=None):
    """Forward of the reference (dtype None: exact) on the inputs of _whh / _xproj; the exact one is shared by the three modes."""
    return bilstm(_xproj(B, T, H, xseed), _whh(H, wseed), lengths=None if lengths is None else list(lengths), dtype=dtype)[0]


def _pack(whh, mode):
    from sos_amd import engine as E
    H = whh.shape[2]
    m = torch.nn.LSTM(4, H, bidirectional=True)
    with torch.no_grad():
        m.weight_hh_l0.copy_(whh[0])
        m.weight_hh_l0_reverse.copy_(whh[1])
    return E.lstm_pack(m.cuda(), mode == "bf16x3")


class _Out:
    """The 16-bit output buffer [B][T][nseg * cs] of sos_lstm_bidir_fwd (thirds hi | hi | lo in bf16x3), pre-filled with
    SENT, followed by a guard of SENT as long as the rows of the partial group's missing clips (+ one clip)."""

    def __init__(self, B, T, H, cs, x3):
        from sos_amd import engine as E
        self.B, self.T, self.H, self.cs, self.nseg = B, T, H, cs, 3 if x3 else 1
        self.row = self.nseg * cs
        self.n = B * T * self.row
        self.t = torch.full((self.n + (_ceil16(B) - B + 1) * T * self.row,), SENT, dtype=E.act_dtype(), device="cuda")

    def rows(self):
        return self.t[:self.n].view(self.B, self.T, self.row).float().cpu()

    def value(self):
        """h as the buffer holds it: hi (+ lo), [B][T][2H]."""
        v = self.rows()
        h = v[..., :2 * self.H]
        return h + v[..., 2 * self.cs:2 * self.cs + 2 * self.H] if self.nseg == 3 else h

    def check_edges(self, written):
        """Channels [2H, cs) of every third keep SENT, the guard keeps SENT, in bf16x3 the second third is the first;
        written [B][T] bool: rows that are outputs (others keep SENT in every channel)."""
        v = self.rows()
        for s in range(self.nseg):
            th = v[..., s * self.cs:(s + 1) * self.cs]
            assert bool((th[..., 2 * self.H:] == SENT).all()), f"channels past 2H written (third {s})"
            assert bool((th[~written] == SENT).all()), f"rows past a clip's length written (third {s})"
        if self.nseg == 3:
            assert torch.equal(v[..., :self.cs][written], v[..., self.cs:2 * self.cs][written])
        assert bool((self.t[self.n:] == SENT).all()), "written past the last clip's rows"


def _fwd(xp, wpk, B, T, H, cs, mode, save=True, lengths=None):
    """One sos_lstm_bidir_fwd launch.  Returns (out, gates, csave) -- gates / csave: the f32 buffers (ceil16(B) clips + guard)."""
    from sos_amd import _lib as L
    out = _Out(B, T, H, cs, mode == "bf16x3")
    gates = csave = None
    if save:
        gates = torch.full((_ceil16(B) * T * 2 * 4 * H + GUARD_F32,), SENT, dtype=torch.float32, device="cuda")
        csave = torch.full((_ceil16(B) * T * 2 * H + GUARD_F32,), SENT, dtype=torch.float32, device="cuda")
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    rc = L.lib().sos_lstm_bidir_fwd(L.ptr(xp), L.ptr(wpk["fh"]), L.ptr(wpk["fl"]), B, T, H, L.ptr(out.t), out.row,
                                    L.DT_BF16X3 if mode == "bf16x3" else L.DT_BF16, cs, L.ptr(gates), L.ptr(csave), L.ptr(lens),
                                    L.stream_ptr())
    L.check(rc, "sos_lstm_bidir_fwd")
    torch.cuda.synchronize()
    if save:
        assert bool((gates[-GUARD_F32:] == SENT).all()) and bool((csave[-GUARD_F32:] == SENT).all()), \
            "saved gates / cell state written past ceil16(B) clips"
    return out, gates, csave


# name (the path it reaches), H, B, T, out_cs extra channels per third.  KF = ceil(H / 32) k-fragments, NT = H / 4 tiles over 8
# waves.  16-bit modes: H = 100 / 200 resident, every other H streamed; bf16x3: the three-pass kernel for all.
CASES = [
    ("H100 resident KF4 elem-store B17 T178", 100, 17, 178, 16),
    ("H100 resident KF4 elem-store B1 T1", 100, 1, 1, 0),
    ("H200 resident KF7 vec-store B64 T178", 200, 64, 178, 0),
    ("H200 resident KF7 vec-store B17 T2", 200, 17, 2, 16),
    ("H4 stream one-tile seven-idle-waves B1 T2", 4, 1, 2, 8),
    ("H4 stream one-tile B17 T178", 4, 17, 178, 0),
    ("H36 stream 2-or-1-tiles elem-store B17 T178", 36, 17, 178, 8),
    # a wave with an odd tile count >= 3: its last prefetch (the next step's first tile) lands in the second buffer
    ("H84 stream KF3 3-tile-waves wrap-around elem-store B17 T178", 84, 17, 178, 8),
    ("H152 stream KF5 5-tile-waves wrap-around vec-store B37 T178", 152, 37, 178, 0),
    ("H64 stream KF2 vec-store B64 T1", 64, 64, 1, 0),
    ("H64 stream KF2 vec-store B17 T178", 64, 17, 178, 16),
    ("H256 stream KF8 eight-tiles B17 T178", 256, 17, 178, 0),
]


def _cs(H, extra):
    return (2 * H + 7) // 8 * 8 + extra


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward(case, mode):
    _, H, B, T, extra = case
    cs = _cs(H, extra)
    seeds = (10 + H, 20 + H + B + T)
    whh, xp = _whh(H, seeds[0]), _xproj(B, T, H, seeds[1])
    out, _, _ = _fwd(xp.cuda(), _pack(whh, mode), B, T, H, cs, mode)
    out.check_edges(torch.ones(B, T, dtype=torch.bool))
    h_ex = _ref_h(H, B, T, *seeds)
    h_m = None if mode == "bf16x3" else _ref_h(H, B, T, *seeds, dtype=_storage(mode))
    s = float(h_ex.abs().max())
    _check(mode, "h", _rel(out.value(), h_ex, s), None if h_m is None else _rel(h_m, h_ex, s))


def test_forward_streaming_w_hh_forced():
    """H = 100 and 200 with W_hh streamed from L2 instead of resident (SOS_LSTM_STREAM_W, read once per process: a child process).
    H = 200: 7 tiles on waves 0-1 and 6 on the others (both sides of the prefetch's wrap-around fix-up); H = 100: 4 and 3."""
    env = dict(os.environ, SOS_LSTM_STREAM_W="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_lstm.py"),
                        "-k", "(test_forward or test_ragged or test_backward) and (H100 or H200) and not bf16x3 and not streaming"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " failed" not in r.stdout, r.stdout[-2000:]


def _ragged_lengths(B, T, seed):
    """Per-clip lengths in [1, T]: 1, 2, T-1 and T mixed within a group and across groups; the last (partial) group's longest
    clip is shorter than T (the group runs to its own longest clip)."""
    lo = max(1, T // 10)
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, T + 1, size=B)
    for b, v in {0: 1, 1: T, 3: 2, 7: T - 1, 16: T - 1, 18: 1, 25: T, 29: 2}.items():
        if b < B:
            lens[b] = v
    if B > 32:                                   # last group: clips 32.. < T
        lens[32:] = np.minimum(lens[32:], T - 3)
        lens[32], lens[-1] = 1, T - 2
    return [int(v) for v in lens]


RAGGED = [
    ("H100 elem-store T178", 100, 178, False),
    ("H200 vec-store T178", 200, 178, False),
    ("H200 vec-store T887 lengths 89-887", 200, 887, True),
]


@pytest.mark.parametrize("case", RAGGED, ids=[c[0] for c in RAGGED])
def test_ragged_forward(case, mode):
    """B = 37 (three 16-clip groups, the last partial) with per-clip lengths: rows [0, len) equal the reference of that clip
    alone (lstm_reference's ragged run, pinned to pack_padded_sequence on the CPU); xproj rows past a clip's length are NaN
    (never read) and its output rows past it keep the sentinel (never written)."""
    from sos_amd import _lib as L
    _, H, T, long_clips = case
    B = 37
    lens = [89 + (887 - 89) * b // (B - 1) for b in range(B)] if long_clips else _ragged_lengths(B, T, H)
    if long_clips:
        lens = lens[1::2] + lens[::2]            # mixed within each group
    cs = _cs(H, 16)
    seeds = (30 + H, 40 + H + T)
    whh, xp = _whh(H, seeds[0]), _xproj(B, T, H, seeds[1])
    xn = xp.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    wpk = _pack(whh, mode)
    out, _, _ = _fwd(xn.cuda(), wpk, B, T, H, cs, mode, save=False, lengths=lens)
    written = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    out.check_edges(written)
    got = out.value()
    assert bool(torch.isfinite(got[written]).all())
    h_ex = _ref_h(H, B, T, *seeds, lengths=tuple(lens))
    h_m = None if mode == "bf16x3" else _ref_h(H, B, T, *seeds, lengths=tuple(lens), dtype=_storage(mode))
    s = float(h_ex.abs().max())
    _check(mode, "h", _rel(got[written], h_ex[written], s), None if h_m is None else _rel(h_m[written], h_ex[written], s))
    # lengths with saved activations: refused (an inference feature)
    g = torch.empty(_ceil16(B) * T * 2 * 4 * H, dtype=torch.float32, device="cuda")
    c = torch.empty(_ceil16(B) * T * 2 * H, dtype=torch.float32, device="cuda")
    rc = L.lib().sos_lstm_bidir_fwd(L.ptr(xn.cuda()), L.ptr(wpk["fh"]), L.ptr(wpk["fl"]), B, T, H, L.ptr(out.t), out.row,
                                    L.DT_BF16X3 if mode == "bf16x3" else L.DT_BF16, cs, L.ptr(g), L.ptr(c),
                                    L.ptr(torch.tensor(lens, dtype=torch.int32, device="cuda")), L.stream_ptr())
    assert rc == -22                     # SOS_EINVAL


def _loss_scale(mode, g):
    """engine.GradScale's factor: 2^floor(log2(256 / max|g|)) in IEEE half (max |g| S in [256, 512)), 1 otherwise."""
    if mode != "fp16":
        return 1.0
    return 2.0 ** np.floor(np.log2(256.0 / float(g.abs().max())))


# name, H, B, T, dh_cs extra channels per third
BWD_CASES = [
    ("H100 KF4 B17 T178 dh_cs>2H", 100, 17, 178, 24),
    ("H200 KF7 B64 T178", 200, 64, 178, 0),
    ("H200 KF7 B1 T2 dh_cs>2H", 200, 1, 2, 8),
    ("H4 B1 T2", 4, 1, 2, 0),
    ("H36 B17 T178 dh_cs>2H", 36, 17, 178, 4),
    ("H64 B64 T1", 64, 64, 1, 0),
    ("H256 KB32 largest-LDS B17 T178", 256, 17, 178, 0),
]


@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_backward(case, mode):
    """sos_lstm_bidir_bwd on the saved gates / cell state of the kernel's own forward: dgates against the reference's float64
    autograd, the region past B*T*2*4H untouched.  fp16: dh_out at the loss scale's magnitude, compared scaled."""
    from sos_amd import _lib as L, engine as E
    _, H, B, T, extra = case
    x3 = mode == "bf16x3"
    whh, xp = _whh(H, 50 + H), _xproj(B, T, H, 60 + H + B + T)
    wpk = _pack(whh, mode)
    _, gates, csave = _fwd(xp.cuda(), wpk, B, T, H, _cs(H, 0), mode)
    g = torch.from_numpy(hashed(70 + H + T, (B, T, 2 * H)).astype(np.float32))
    g = g * _loss_scale(mode, g)
    # dh_out as the 16-bit buffer holds it ([B][T][nseg * dcs], lo third at +2 * dcs in bf16x3) and the value it holds
    st, dcs = E.act_dtype(), (2 * H + 3) // 4 * 4 + extra
    nseg = 3 if x3 else 1
    buf = torch.zeros(B, T, nseg * dcs, dtype=st)
    hi = g.to(st)
    buf[..., :2 * H] = hi
    held = hi.float()
    if x3:
        lo = (g - hi.float()).to(st)
        buf[..., dcs:dcs + 2 * H] = hi
        buf[..., 2 * dcs:2 * dcs + 2 * H] = lo
        held = held + lo.float()
    dg = torch.full((B * T * 2 * 4 * H + GUARD_F32,), SENT, dtype=torch.float32, device="cuda")
    L.check(L.lib().sos_lstm_bidir_bwd(L.ptr(buf.cuda()), nseg * dcs, L.DT_BF16X3 if x3 else L.DT_BF16, dcs, L.ptr(gates),
                                       L.ptr(csave), L.ptr(wpk["bh"]), L.ptr(wpk["bl"]), B, T, H, L.ptr(dg), L.stream_ptr()),
            "sos_lstm_bidir_bwd")
    torch.cuda.synchronize()
    dg = dg.cpu()
    assert bool((dg[B * T * 2 * 4 * H:] == SENT).all()), "dgates written past B*T*2*4H"
    got = dg[:B * T * 2 * 4 * H].view(B, T, 2, 4 * H)
    _, d_ex = bilstm(xp, whh, dh_out=held)
    d_m = None if x3 else bilstm(xp, whh, dtype=_storage(mode), dh_out=held)[1]
    s = float(d_ex.abs().max())
    _check(mode, "dgates", _rel(got, d_ex, s), None if d_m is None else _rel(d_m, d_ex, s))


# name, I (input width), B, T, H
TRAIN_CASES = [
    ("I48 H100 B17 T178", 48, 17, 178, 100),
    ("I64 H200 B64 T178", 64, 64, 178, 200),
    ("I64 H100 B64 T1", 64, 64, 1, 100),
    ("I48 H200 B17 T1", 48, 17, 1, 200),
]

TORCH_NAMES = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]


def _train_model(lstm, x, g, st, S, lengths=None):
    """Storage model of the training layer (dtype st, loss scale S; st None: exact): xproj = x q(W_ih)^T + b (f32 conv output),
    the recurrence of lstm_reference, the 16-bit copy of the (scaled) dgates that the weight gradients and the input gradient
    contract, dfeat stored in 16 bits.  Returns h, dfeat and the parameter gradients under torch's names."""
    q = (lambda t: t) if st is None else (lambda t: t.to(st).double())
    B, T, _ = x.shape
    H = lstm.hidden_size
    p = {k: v.detach().double().cpu() for k, v in lstm.named_parameters()}
    wih = torch.cat([p["weight_ih_l0"], p["weight_ih_l0_reverse"]])                                # (8H, I) torch order
    b = torch.cat([p["bias_ih_l0"] + p["bias_hh_l0"], p["bias_ih_l0_reverse"] + p["bias_hh_l0_reverse"]])
    xp = to_kernel_order(x @ q(wih).t() + b, H).view(B, T, 2, 4 * H)
    whh = torch.stack([p["weight_hh_l0"], p["weight_hh_l0_reverse"]])
    h, dg = bilstm(xp, whh, dtype=st, dh_out=g * S)
    dgq = to_torch_order(q(dg.view(B, T, 8 * H)), H)                                                 # scaled, stored
    out = {"h": h, "dfeat": q(dgq @ q(wih)) / S}
    dgq = dgq / S
    for d, sfx in ((0, ""), (1, "_reverse")):
        gd = dgq[..., d * 4 * H:(d + 1) * 4 * H]
        hd = h[..., d * H:(d + 1) * H]
        hp = torch.zeros_like(hd)
        if d == 0:
            hp[:, 1:] = hd[:, :-1]
        else:
            hp[:, :-1] = hd[:, 1:]
        out["weight_ih_l0" + sfx] = torch.einsum("btg,bti->gi", gd, x)
        out["weight_hh_l0" + sfx] = torch.einsum("btg,bth->gh", gd, hp)
        out["bias_ih_l0" + sfx] = out["bias_hh_l0" + sfx] = gd.sum((0, 1))
    return out


@pytest.mark.parametrize("case", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_train_layer(case, mode):
    """train_ops.lstm_train_plan -> lstm_forward_train -> lstm_backward (in fp16 under a GradScale, as the agents run it) against
    torch.nn.LSTM(...).double() on the values the feature matrix holds: h, dfeat and every parameter gradient (unscaled).
    The exact reference is torch's own module; at T = 1 the recurrent weights' gradients are exactly zero."""
    from sos_amd import _lib as L, engine as E, train_ops as TO
    _, I, B, T, H = case
    x3 = mode == "bf16x3"
    st = E.act_dtype()
    dev = torch.device("cuda")
    torch.manual_seed(H + I + T)
    lstm = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True)
    with torch.no_grad():
        for i, (name, prm) in enumerate(lstm.named_parameters()):
            prm.copy_(torch.from_numpy(hashed(100 + 10 * i + H, tuple(prm.shape),
                                              (1.5 if "hh" in name else 0.6) / np.sqrt(prm.shape[1] if prm.dim() == 2 else H))
                                       .astype(np.float32)))
    x = torch.from_numpy(hashed(80 + I + T, (B, T, I)).astype(np.float32) * 2.0)
    hi = x.to(st)
    held = hi.float()
    if x3:
        lo = (x - hi.float()).to(st)
        feat = torch.cat([hi, hi, lo], dim=2)
        held = held + lo.float()
    else:
        feat = hi
    feat = feat.to(dev).contiguous()
    lp = TO.lstm_train_plan(lstm.to(dev), I, x3)
    h, tape = TO.lstm_forward_train(lp, (feat, B, 1, T, I, 3 if x3 else 1), B, T, x3, dev)
    g = torch.from_numpy(hashed(90 + H + T, (B, T, 2 * H)).astype(np.float32)).to(dev)
    grads = {}
    with E.backward_scale(g) as gs:
        dh = E.Act(B, 1, T, E.pad_to(2 * H, 16), x3, dev, zero=True)
        TO.pack_grad(g, None, L.ACT_NONE, B, T, 2 * H, T * 2 * H, 2 * H, 1, dh)
        dfeat = TO.lstm_backward(lp, tape, dh, grads, "lstm", B, T, x3, dev)
    torch.cuda.synchronize()
    S = 1.0 if gs.mul is None else float(gs.mul.cpu())
    assert mode != "fp16" or S > 1.0
    ht = h.t.float().cpu().view(B, T, -1)
    hk = ht[..., :2 * H] + (ht[..., 2 * h.cs:2 * h.cs + 2 * H] if x3 else 0.0)
    dt = dh.t.float().cpu().view(B, T, -1)
    g_held = (dt[..., :2 * H] + (dt[..., 2 * dh.cs:2 * dh.cs + 2 * H] if x3 else 0.0)).double() / S
    df = dfeat.float().cpu()
    got = {"h": hk, "dfeat": (df[..., :I] + (df[..., 2 * I:3 * I] if x3 else 0.0)).double() / S}
    for n in TORCH_NAMES:
        for sfx in ("", "_reverse"):
            got[n + sfx] = grads["lstm." + n + sfx].detach().double().cpu()
    # exact: torch's module in float64
    ref = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in lstm.state_dict().items()})
    xd = held.double().requires_grad_(True)
    y, _ = ref(xd)
    y.backward(g_held)
    exact = {"h": y.detach(), "dfeat": xd.grad}
    for n, prm in ref.named_parameters():
        exact[n] = prm.grad
    model = None if x3 else _train_model(lstm, held.double(), g_held, st, S)
    for k, want in exact.items():
        if T == 1 and k.startswith("weight_hh"):
            assert not got[k].any(), f"{k}: no previous state at T = 1, its gradient must be exactly zero"
            continue
        s = float(want.abs().max())
        what = "h" if k == "h" else "grad"
        _check(mode, what, _rel(got[k], want, s), None if model is None else _rel(model[k], want, s))
