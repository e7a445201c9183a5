"""TEST INFRASTRUCTURE: a plain float64 bidirectional LSTM at the boundary of the recurrent kernels (include/sos_hip.h,
sos_lstm_bidir_fwd / sos_lstm_bidir_bwd): the input projection `xproj` is given, in the ABI's gate-interleaved layout
[B][T][2][4H] (channel dir*4H + 4*j + q for hidden unit j, gate q in i,f,g,o), W_hh in torch's [2][4H][H].

`bilstm(xproj, whh, lengths, dtype, dh_out)` returns the output h [B][T][2H] and, for a given dh_out [B][T][2H], dgates =
d(sum(h * dh_out)) / d(xproj) [B][T][2][4H] (gate-interleaved), taken by float64 autograd with xproj as the leaf.

lengths (optional, [B]): clip b runs over frames [0, lengths[b]) in both directions -- the reverse pass starts at the clip's own
last frame, as pack_padded_sequence does; rows past a clip's length are 0 in h and dgates.

dtype (optional, torch.float16 / torch.bfloat16): round trips through the 16-bit storage type where the kernels STORE in 16
bits (tests/storage_model.py's rule): W_hh, the stored h_t (the output, and the B operand of the next step's recurrent product),
dh_out, and the 16-bit copy of dgates_t that is the B operand of the backward's recurrent product dh_rec = W_hh^T dgates_t.
Gate arithmetic, the cell state and every accumulator stay unrounded (float64 here).  dtype=None: the exact reference."""
import torch


def _q(x, dtype):
    return x if dtype is None else x.to(dtype).to(torch.float64)


class _RoundFwd(torch.autograd.Function):
    """Stored h_t: rounded in forward, the gradient passes unrounded (the kernel adds dh_out + dh_rec in f32)."""

    @staticmethod
    def forward(ctx, x, dtype):
        return _q(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _RoundBwd(torch.autograd.Function):
    """The recurrent product's output: identity in forward; its gradient (dgates_t) is rounded before it is multiplied
    by W_hh^T (the kernel's 16-bit LDS copy of dgates_t)."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return _q(g, ctx.dtype), None


def to_torch_order(x, H):
    """Gate-interleaved [..., 2*4H] (dir, j, q) -> torch's (dir, q, j) order (engine.lstm_gate_perm)."""
    from sos_amd import engine as E
    _, inv = E.lstm_gate_perm(H, x.device)
    return x[..., inv]


def to_kernel_order(x, H):
    """torch's (dir, q, j) order [..., 8H] -> gate-interleaved (dir, j, q)."""
    from sos_amd import engine as E
    perm, _ = E.lstm_gate_perm(H, x.device)
    return x[..., perm]


def bilstm(xproj, whh, lengths=None, dtype=None, dh_out=None):
    """See the module docstring.  xproj [B][T][2][4H] (gate-interleaved), whh [2][4H][H] (torch order, both directions),
    lengths [B] ints or None, dh_out [B][T][2H] or None.  Returns (h, dgates or None), float64 on the CPU."""
    xproj = torch.as_tensor(xproj).detach().to("cpu", torch.float64)
    whh = torch.as_tensor(whh).detach().to("cpu", torch.float64)
    B, T, _, G = xproj.shape
    H = G // 4
    assert whh.shape == (2, G, H), whh.shape
    lens = torch.full((B,), T, dtype=torch.long) if lengths is None else torch.as_tensor(lengths, dtype=torch.long).cpu()
    assert int(lens.min()) >= 1 and int(lens.max()) <= T
    leaf = xproj.clone().requires_grad_(dh_out is not None)
    xt = to_torch_order(leaf.reshape(B, T, 2 * G), H).reshape(B, T, 2, 4, H)     # [b][t][dir][gate][unit]
    steps = torch.arange(T)
    active = steps[None, :] < lens[:, None]                                         # [B][step]
    outs = []
    for d in range(2):
        w = _q(whh[d], dtype)
        # time index of step s: s (forward), lengths[b] - 1 - s (reverse; clamped where the clip has ended)
        tix = steps[None, :].expand(B, T) if d == 0 else (lens[:, None] - 1 - steps[None, :]).clamp(min=0)
        xs = xt[:, :, d][torch.arange(B)[:, None], tix]                            # [B][step][4][H]
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        hs = []
        for s in range(T):
            a = xs[:, s] + _RoundBwd.apply(h @ w.t(), dtype).view(B, 4, H)
            i, f, g, o = torch.sigmoid(a[:, 0]), torch.sigmoid(a[:, 1]), torch.tanh(a[:, 2]), torch.sigmoid(a[:, 3])
            c_new = f * c + i * g
            h_new = _RoundFwd.apply(o * torch.tanh(c_new), dtype)
            if lengths is None:
                c, h = c_new, h_new
                hs.append(h_new)
                continue
            m = active[:, s, None]
            c = torch.where(m, c_new, c)
            h = torch.where(m, h_new, h)
            hs.append(torch.where(m, h_new, torch.zeros_like(h_new)))
        hs = torch.stack(hs, 1)                                                     # [B][step][H]
        if d == 1 and lengths is None:                                              # step order -> time order
            hs = hs.flip(1)
        elif d == 1:
            out = torch.zeros(B, T, H, dtype=torch.float64)
            for b in range(B):
                n = int(lens[b])
                out[b, :n] = hs[b, :n].flip(0)
            hs = out
        outs.append(hs)
    h = torch.cat(outs, dim=2)                                                      # [B][T][2H]
    if dh_out is None:
        return h.detach(), None
    dh = _q(torch.as_tensor(dh_out).detach().to("cpu", torch.float64), dtype)
    h.backward(dh)
    return h.detach(), leaf.grad.detach()
