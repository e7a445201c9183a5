"""CPU pin of tests/lstm_reference.py (the float64 oracle of the recurrent kernels, tests/test_gpu_lstm.py) against torch.nn.LSTM:
forward in both directions, ragged batches against pack_padded_sequence, the gate gradients against torch's parameter
gradients, and the storage-rounding variant."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from lstm_reference import bilstm, to_kernel_order, to_torch_order

B, T, I, H = 5, 9, 7, 12
LENGTHS = [9, 1, 4, 2, 8]


def _module(seed=0):
    torch.manual_seed(seed)
    m = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():                    # weights and inputs large enough that some gates saturate and others do not
        for p in m.parameters():
            p.mul_(4.0)
    x = torch.randn(B, T, I, dtype=torch.float64)
    return m, x


def _xproj(m, x):
    """x @ W_ih^T + b_ih + b_hh of both directions, in the kernels' gate-interleaved layout [B][T][2][4H]."""
    parts = [x @ getattr(m, "weight_ih_l0" + s).t() + getattr(m, "bias_ih_l0" + s) + getattr(m, "bias_hh_l0" + s)
             for s in ("", "_reverse")]
    return to_kernel_order(torch.cat(parts, dim=2), H).reshape(B, T, 2, 4 * H).detach()


def _whh(m):
    return torch.stack([m.weight_hh_l0, m.weight_hh_l0_reverse]).detach()


def test_gate_order_round_trip():
    v = torch.randn(3, 8 * H, dtype=torch.float64)
    assert torch.equal(to_torch_order(to_kernel_order(v, H), H), v)
    # gate-interleaved: channel dir*4H + 4j + q holds torch's dir*4H + q*H + j
    k = to_kernel_order(v, H)
    for d, j, q in ((0, 0, 0), (0, 5, 2), (1, 11, 3), (1, 3, 1)):
        assert k[0, d * 4 * H + 4 * j + q] == v[0, d * 4 * H + q * H + j]


def test_forward_equals_torch_lstm():
    m, x = _module()
    want = m(x)[0].detach()
    got, _ = bilstm(_xproj(m, x), _whh(m))
    assert got.shape == (B, T, 2 * H)
    assert float((got - want).abs().max()) < 1e-12
    assert float(want[..., H:].abs().max()) > 0.5 and float(want[..., :H].abs().max()) > 0.5     # both directions non-trivial


def test_ragged_forward_equals_packed_sequence():
    m, x = _module(1)
    packed = pack_padded_sequence(x, torch.tensor(LENGTHS), batch_first=True, enforce_sorted=False)
    want, _ = pad_packed_sequence(m(packed)[0], batch_first=True, total_length=T)
    got, _ = bilstm(_xproj(m, x), _whh(m), lengths=LENGTHS)
    assert float((got - want.detach()).abs().max()) < 1e-12
    for b, n in enumerate(LENGTHS):
        assert not got[b, n:].any()
        # the reverse direction starts at the clip's own last frame: not the same as the padded full-length run
        full, _ = m(x[b:b + 1, :n])
        assert float((got[b, :n] - full[0].detach()).abs().max()) < 1e-12


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_dgates_give_torch_parameter_gradients(ragged):
    m, x = _module(2)
    lengths = LENGTHS if ragged else [T] * B
    dh = torch.randn(B, T, 2 * H, dtype=torch.float64)
    for b, n in enumerate(lengths):
        dh[b, n:] = 0.0
    if ragged:
        packed = pack_padded_sequence(x, torch.tensor(lengths), batch_first=True, enforce_sorted=False)
        y, _ = pad_packed_sequence(m(packed)[0], batch_first=True, total_length=T)
    else:
        y, _ = m(x)
    (y * dh).sum().backward()
    h, dg = bilstm(_xproj(m, x), _whh(m), lengths=lengths if ragged else None, dh_out=dh)
    dg = to_torch_order(dg.reshape(B, T, 8 * H), H).reshape(B, T, 2, 4 * H)
    for d, sfx in ((0, ""), (1, "_reverse")):
        g = dg[:, :, d]                                                            # [B][T][4H], torch gate order
        hd = h[..., d * H:(d + 1) * H]
        # previous state: h[t-1] (forward), h[t+1] (reverse; zero past the clip's last frame), 0 at the first step
        hp = torch.zeros_like(hd)
        if d == 0:
            hp[:, 1:] = hd[:, :-1]
        else:
            hp[:, :-1] = hd[:, 1:]
        want = {"weight_ih_l0": torch.einsum("btg,bti->gi", g, x), "bias_ih_l0": g.sum((0, 1)), "bias_hh_l0": g.sum((0, 1)),
                "weight_hh_l0": torch.einsum("btg,bth->gh", g, hp)}
        for name, w in want.items():
            ref = getattr(m, name + sfx).grad
            assert float((w - ref).abs().max()) < 1e-10 * float(ref.abs().max()), name + sfx


def test_single_frame_has_no_recurrent_gradient():
    m, x = _module(3)
    x1 = x[:, :1]
    xp = _xproj(m, x)[:, :1]
    dh = torch.randn(B, 1, 2 * H, dtype=torch.float64)
    y, _ = m(x1)
    (y * dh).sum().backward()
    assert not m.weight_hh_l0.grad.any() and not m.weight_hh_l0_reverse.grad.any()
    _, dg = bilstm(xp, _whh(m), dh_out=dh)
    assert dg.abs().max() > 0


def test_rounding_variant_reduces_to_exact():
    m, x = _module(4)
    dh = torch.randn(B, T, 2 * H, dtype=torch.float64)
    h0, g0 = bilstm(_xproj(m, x), _whh(m), lengths=LENGTHS, dh_out=dh)
    h1, g1 = bilstm(_xproj(m, x), _whh(m), lengths=LENGTHS, dtype=torch.float64, dh_out=dh)
    assert torch.equal(h0, h1) and torch.equal(g0, g1)


@pytest.mark.parametrize("dtype,lo,hi", [(torch.float16, 1e-5, 3e-3), (torch.bfloat16, 1e-4, 3e-2)], ids=["fp16", "bf16"])
def test_rounding_variant_rounds_where_the_kernels_store(dtype, lo, hi):
    """The stored h_t is representable in the storage type; the model's deviation from the exact reference is the size of
    that format's rounding (relative to max |h| / max |dgates|), not zero and not more."""
    m, x = _module(5)
    dh = torch.randn(B, T, 2 * H, dtype=torch.float64)
    h0, g0 = bilstm(_xproj(m, x), _whh(m), dh_out=dh)
    h1, g1 = bilstm(_xproj(m, x), _whh(m), dtype=dtype, dh_out=dh)
    assert torch.equal(h1.to(dtype).double(), h1)
    eh = float((h1 - h0).abs().max() / h0.abs().max())
    eg = float((g1 - g0).abs().max() / g0.abs().max())
    assert lo < eh < hi and lo < eg < hi, (eh, eg)
    # only dh_out rounded (a value already in the storage type is left as it is)
    dq = dh.to(dtype).double()
    _, g2 = bilstm(_xproj(m, x), _whh(m), dtype=dtype, dh_out=dq)
    assert torch.equal(g1, g2)
