"""tests/train_reference.py pinned on the CPU: the losses against torch's float64 losses and autograd, adam_step against
torch.optim.Adam on float64 parameters, loss_scale against tests/storage_model.py's float64 rule, gather_pack against
Tensor.to(bfloat16 / float16), the guard's state machine on the sequences the GPU test replays -- and the format model
adam_step_f32 is shown to be a usable yardstick on every case of the GPU test's grid."""
import numpy as np
import pytest
import torch

import train_reference as R
from storage_model import loss_scale_for


def _rng_pair(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n)


@pytest.mark.parametrize("upstream", [1.0, 3.0, 0.37])
def test_losses_match_torch_float64(upstream):
    a, b = _rng_pair(1237, 1)
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    l = torch.nn.functional.mse_loss(ta, torch.tensor(b, dtype=torch.float64))
    (R.f32(upstream) * l).backward()
    loss, grad = R.mse(a, b, upstream)
    assert abs(loss - l.item()) <= 1e-14 * abs(l.item()) and np.max(np.abs(grad - ta.grad.numpy())) <= 1e-15 * np.max(np.abs(grad))
    x = np.concatenate([4.0 * a, [0.0, 1e-4, -1e-4, 20, -20, 88, -88, 104, -104, 200, -200]])
    y = np.concatenate([(b > 0).astype(np.float64), [0.3, 0, 1, 0.3, 0, 1, 0.3, 0, 1, 0.3, 0.3]])
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    l = torch.nn.functional.binary_cross_entropy_with_logits(tx, torch.tensor(y, dtype=torch.float64))
    (R.f32(upstream) * l).backward()
    loss, grad = R.bce_logits(x, y, upstream)
    assert abs(loss - l.item()) <= 1e-14 * abs(l.item()) and np.max(np.abs(grad - tx.grad.numpy())) <= 1e-15 * np.max(np.abs(grad))
    assert np.isfinite(grad).all()


def test_loss_accumulation_bound_counts_the_trips():
    assert R.loss_accumulation_bound(1) == 12 * 2.0 ** -24 and R.loss_accumulation_bound(262144) == 12 * 2.0 ** -24
    assert R.loss_accumulation_bound(262145) == 13 * 2.0 ** -24 and R.loss_accumulation_bound(R.N1) == 14 * 2.0 ** -24


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step_iterated_matches_torch_adam(wd):
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(501)
    tp = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    h = R.ADAM_HYPER
    # torch receives the hyper-parameters as the C ABI does: rounded to float
    opt = torch.optim.Adam([tp], lr=R.f32(h["lr"]), betas=(R.f32(h["b1"]), R.f32(h["b2"])), eps=R.f32(h["eps"]), weight_decay=R.f32(wd))
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 21):
        g = rng.standard_normal(501) * 10.0 ** rng.integers(-8, 1)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, m, v = R.adam_step(p, g, m, v, h["lr"], h["b1"], h["b2"], h["eps"], wd, step, 1.0)
        st = opt.state[tp]
        assert R.update_error(p, tp.detach().numpy(), p0) <= 1e-12
        assert R.max_rel(m, st["exp_avg"].numpy()) <= 1e-12 and R.max_rel(v, st["exp_avg_sq"].numpy()) <= 1e-12


def test_adam_step_scales_the_gradient_and_counts_applied_steps():
    p, g, m, v = (a.astype(np.float64) for a in R.adam_case(5, 300, 1e-4, 1.0, False))
    h = R.ADAM_HYPER
    want = R.adam_step(p, 0.125 * g, m, v, wd=0.01, step=7, grad_scale=1.0, **h)
    for got in (R.adam_step(p, g, m, v, wd=0.01, step=10, grad_scale=0.125, skipped=3, **h),):
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    at1 = R.adam_step(p, g, m, v, wd=0.0, step=1, grad_scale=1.0, **h)
    assert all(np.array_equal(a, b) for a, b in zip(R.adam_step(p, g, m, v, wd=0.0, step=4, grad_scale=1.0, skipped=9, **h), at1))


def test_adam_format_model_is_a_usable_yardstick_on_every_case():
    """The GPU test bounds the kernel's update error by 4 x the float32 model's own: the model's has to be small for that to mean
    anything (a badly chosen case cannot loosen the bound), and m, v of the model stay inside the derived 8 * 2^-24."""
    h = R.ADAM_HYPER
    worst = {1.0: 0.0, 1e-3: 0.0}
    for c in R.adam_grid():
        p, g, m, v = R.adam_case(c["seed"], 1500, c["g_scale"], c["p_scale"], c["step"] == 1)
        args = dict(wd=c["wd"], step=c["step"], grad_scale=c["grad_scale"], **h)
        ref = R.adam_step(p, g, m, v, **args)
        mod = R.adam_step_f32(p, g, m, v, **args)
        e = R.update_error(mod[0], ref[0], p)
        worst[c["p_scale"]] = max(worst[c["p_scale"]], e)
        assert 0.0 < e < R.ADAM_MODEL_E_MAX[c["p_scale"]], (c, e)
        assert R.max_rel(mod[1], ref[1]) <= 8 * 2.0 ** -24 and R.max_rel(mod[2], ref[2]) <= 8 * 2.0 ** -24, c
        assert np.min(ref[2]) >= 2.0 ** -126, c                                     # v stays a normal float32
    print("adam format model: worst E", worst)


def test_loss_scale_equals_the_float64_rule_at_every_power_of_two_edge():
    for a in R.loss_scale_amax_values():
        S, inv = R.loss_scale(a, 256.0)
        assert S == loss_scale_for(torch.tensor([-float(a), 0.0])), a
        assert S * inv == 1.0
        assert S * float(a) <= 256.0 or S == 2.0 ** -40
        assert 2.0 * S * float(a) > 256.0 or S == 2.0 ** 40
    # the predicted edge: one float32 above 2^-3 the scale is 2^10, not 2^11
    assert R.loss_scale(np.nextafter(np.float32(0.125), np.float32(1)), 256.0) == (1024.0, 1.0 / 1024.0)
    assert R.loss_scale(0.125, 256.0)[0] == 2048.0
    # any target: S a <= T < 2 S a, in exact arithmetic (a power of two times a float32 is exact in float64), at the target's own edges
    for j in range(-45, 46, 5):
        for a in R.neighbours(np.float32(100.0) * np.float32(2.0 ** j)):
            S, _ = R.loss_scale(a, 100.0)
            assert (S * float(a) <= 100.0 or S == 2.0 ** -40) and (2.0 * S * float(a) > 100.0 or S == 2.0 ** 40), (j, a)
    # why the GPU test walks these edges: floor(log2(q)) with q and log2 correctly rounded to float32 is NOT this rule
    wrong = 0
    for j in range(-30, 31):
        a = np.float32(2.0 ** j)
        for _ in range(6):
            a = np.nextafter(a, np.float32(np.inf), dtype=np.float32)
            e = int(np.floor(np.float32(np.log2(np.float64(np.float32(256.0) / a)))))
            wrong += 2.0 ** e != R.loss_scale(a, 256.0)[0]
    assert wrong == 191
    for a in (0.0, 3.2e38, np.inf, np.nan):
        assert R.loss_scale(a, 256.0) == (1.0, 1.0)
    assert R.loss_scale(1.0, 100.0)[0] == 64.0 and R.loss_scale(100.0, 100.0)[0] == 1.0
    assert R.loss_scale(1.0, 256.0, 0.0) == R.loss_scale(1.0, 256.0) == R.loss_scale(1.0, 256.0, None)
    assert R.loss_scale(1.0, 256.0, 0.5)[0] == 128.0 and R.loss_scale(1.0, 256.0, 2.0 ** -20)[0] == 2.0 ** -12


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gather_pack_equals_torch_casts_bit_for_bit(dtype):
    td = torch.bfloat16 if dtype == "bf16" else torch.float16
    v = R.pack_values(dtype)
    t = torch.from_numpy(v)
    hi = t.to(td)
    lo = (t - hi.float()).to(td)
    hi, lo = (h.view(torch.int16).numpy().view(np.uint16) for h in (hi, lo))
    kinds = np.arange(v.size) % 3 - 1
    for shift in range(3):          # every value under every kind
        k = np.roll(kinds, shift)
        want = np.where(k > 0, hi, np.where(k < 0, lo, np.uint16(0)))
        got = R.gather_pack(v, k, dtype)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (dtype, v[bad[:5]], got[bad[:5]], want[bad[:5]])
    if dtype == "fp16":             # the edges do what they are there for
        assert list(R.to_storage_bits(np.array([65519.0, 65520.0, 2.0 ** -25, 3 * 2.0 ** -25], np.float32), dtype)) == [0x7BFF, 0x7C00, 0, 2]
    else:
        assert R.to_storage_bits(np.array([np.finfo(np.float32).max], np.float32), dtype)[0] == 0x7F80


def test_is_bad_is_the_exponent_test():
    bits = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F7FFFFF, 0xFF7FFFFF, 0, 0x80000000, 1, 0x007FFFFF],
                    dtype=np.uint32)
    assert list(R.is_bad(bits)) == [True] * 5 + [False] * 6
    assert list(R.is_bad(bits)) == list(~np.isfinite(bits.view(np.float32)))


def test_guard_state_machine_sequences():
    s = [0.0, 0.0, 0.0, 0.0, 0]
    for k in range(1, 23):                                  # 22 overflows in a row: halved from "0 reads as 1" down to the floor
        s = R.guard_finalize(s, True)
        assert s == [1.0, max(2.0 ** -k, 2.0 ** -20), 0.0, float(k), 0]
    for k in range(1, 401):                                 # 200 and 400 finite steps: one doubling each, counter reset
        s = R.guard_finalize(s, False)
        assert s == [0.0, 2.0 ** -20 * (1 + (k >= 200) + 2 * (k >= 400)), float(k % 200), 22.0, 0]
    s = [0.0, 0.5, 199.0, 3.0, 0]
    s = R.guard_finalize(s, False)
    assert s == [0.0, 1.0, 0.0, 3.0, 0]
    for k in range(1, 402):                                 # growth stops at 1: the counter just counts
        s = R.guard_finalize(s, False)
        assert s == [0.0, 1.0, float(k), 3.0, 0]
    assert R.guard_finalize([0.0, 1.0, 5.0, 0.0, 1], False) == [1.0, 0.5, 0.0, 1.0, 0]      # a flag left by an earlier scan counts
    assert R.guard_finalize([1.0, -1.0, 5.0, 2.0, 0], False) == [0.0, 1.0, 6.0, 2.0, 0]
