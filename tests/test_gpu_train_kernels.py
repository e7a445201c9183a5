"""The training-step kernels of csrc/train.hip, each through the C ABI, against the float64 / exact-integer references of
tests/train_reference.py at the sizes where their launches change shape:

  sos_mse_loss, sos_bce_logits_loss       1024-block grid cap: n up to N1 = 2 * 262144 + 257 (threads take 2 or 3 trips)
  sos_amax_f32, sos_loss_scale, sos_scale_f32 (2048-block cap: N2 = 524288 + 300)
  sos_grad_guard                          scan at N1, the state machine step by step
  sos_adam_step, sos_adam_multi_step      one step from a given state; tensors of every chunk-edge size in one launch
  sos_gather_pack_multi                   in the bf16 and the fp16 build

Every output buffer lies inside a larger allocation between 64-word runs of a NaN bit pattern (Carved), compared as integers
after the call.  Bounds are derived (train_reference.loss_accumulation_bound; roundings counted next to each assertion) or are
4 x the error of the same formula evaluated in numpy float32 (the device's expf / log1pf / powf are accurate to a few ulp, not
correctly rounded); exact where the result is exactly defined (amax, loss scale, scale, guard, packing, skipped steps).

Observed on MI355X (printed by the tests as `train-err`), next to the bound:
  MSE loss, relative          1.8e-8 .. 4.4e-8 over the seven sizes (1.8e-8 at N1)    bound 7.2e-7 .. 8.3e-7 ((k + 11) 2^-24)
  MSE gradient, per element   <= 1.6e-7 (2.6 units of 2^-24)                          bound 3.0e-7 (5 * 2^-24)
  BCE loss, relative          2.3e-10 .. 3.0e-8 (1.4e-8 at N1)                        bound 1.3e-6 .. 1.9e-6 (E_term 1.6e-7 .. 2.9e-7)
  BCE gradient, max-norm      8.4e-8 .. 1.5e-7, 0.92 .. 1.02 x the float32 model's    bound 4 x the model's
  BCE edge logits             loss 9.1e-8 (summed-term bound 7.5e-7; E_term is 1 there: exp(-104) is below float32's range, so
                              the per-term bound says nothing and the summed one is asserted as well); gradient 1.00 x the model's
  Adam m / v, max-norm        <= 2.4 / 3.2 units of 2^-24                              bound 8
  Adam update E               worst of a step's 36 cases 3.2e-5 .. 2.7e-4 (the |p| ~ 1 cases: p's own grid); the worst ratio to
                              the model's E per step 1.06 .. 1.28                      bound 4 x the model's
  sos_adam_step at N2         E 1.8e-7 (model 1.7e-7), m 0.6, v 0.7 units
  FusedAdam, three steps      E 1.5e-6 (model 1.5e-6)
  amax, loss scale, scale, guard, skipped-step no-op, multi- vs single-tensor Adam, packing: exact, no figure.
The whole file takes 5 s.
"""
import functools

import numpy as np
import pytest
import torch

import train_reference as R
from util import hashed

pytestmark = pytest.mark.gpu

# The float32 sentinel is a SIGNALLING NaN: Adam and sos_scale_f32 update in place, and an update of a quiet NaN returns that
# NaN, payload and all -- the same bits, so a kernel running past its tensor would leave quiet-NaN sentinels `intact'.
# Arithmetic on a signalling NaN sets the quiet bit.  (Measured: with quiet NaNs the chunk bound `hi` of adam_multi_kernel
# replaced by lo + SOS_ADAM_CHUNK passed every test.)  The multi-tensor test runs once more between FINITE sentinels.
SENT32 = 0x7F800BAD
SENT32_FINITE = 0x3F800BAD  # 1.0003555: any Adam update moves it
SENT16 = 0x7FC1             # a NaN in bfloat16 and in IEEE half (the 16-bit outputs are stored, never updated)
H = R.ADAM_HYPER
U24 = 2.0 ** -24


def _L():
    from sos_amd import _lib as L
    return L


def _call(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*args, L.stream_ptr()), name)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(word):
    return int(np.array(word, dtype=np.uint32).view(np.int32))


class Carved:
    """Tensors of `sizes` elements carved from ONE allocation: 64 sentinel words (int32; 128 elements for the 16-bit kind) before,
    between and after them, `tail` more sentinel elements at the end (a chunk that ran past its tensor would land there, not
    outside the allocation).  view(i): tensor i (float32 / int16); intact(): every sentinel still holds its bits."""

    def __init__(self, sizes, tail=0, dtype=torch.int32, sent=None):
        self.dtype, self.sent = dtype, sent if sent is not None else (SENT32 if dtype == torch.int32 else SENT16)
        pad = 64 if dtype == torch.int32 else 128
        self.offs, o = [], pad
        for s in sizes:
            self.offs.append(o)
            o += s + pad
        self.sizes = list(sizes)
        self.raw = torch.full((o + tail,), self.sent, dtype=dtype, device="cuda")
        self.inside = torch.zeros(o + tail, dtype=torch.bool, device="cuda")
        for off, s in zip(self.offs, sizes):
            self.inside[off:off + s] = True

    def view(self, i=0):
        r = self.raw[self.offs[i]:self.offs[i] + self.sizes[i]]
        return r.view(torch.float32) if self.dtype == torch.int32 else r

    def ptr(self, i=0):
        return self.raw.data_ptr() + self.raw.element_size() * self.offs[i]

    def put(self, i, a):
        self.view(i).copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return self

    def get(self, i=0):
        return self.view(i).cpu().numpy()

    def intact(self):
        return bool((self.raw[~self.inside] == self.sent).all())


# ================================================================================================================= losses
LOSS_N = (1, 255, 256, 257, 262144, 262145, R.N1)
UPSTREAMS = (1.0, 3.0, 0.37)
LOSS_FN = {"mse": "sos_mse_loss", "bce": "sos_bce_logits_loss"}


@functools.lru_cache(maxsize=None)
def _loss_inputs(kind, n):
    """float32 (a, b) / (x, y).  MSE: |a - b| in [0.25, 1], so every gradient element is a normal number.  BCE: logits 4 N(0, 1),
    hard labels."""
    if kind == "mse":
        a = hashed(11, (n,)).astype(np.float32)
        d = hashed(12, (n,))
        b = (a.astype(np.float64) - np.where(d < 0, -1.0, 1.0) * (0.25 + 0.75 * np.abs(d))).astype(np.float32)
        return a, b
    rng = np.random.default_rng(100 + n)
    return (4.0 * rng.standard_normal(n)).astype(np.float32), (rng.random(n) < 0.5).astype(np.float32)


def _run_loss(kind, da, db, upstream, with_grad=True):
    """One launch on device tensors -> (loss float32, gradient Carved or None); asserts that nothing else was written: the
    sentinels around loss, partial and grad, and the partial sums of the blocks the grid does not have."""
    n = da.numel()
    loss, partial = Carved([1]), Carved([1024])          # (the carved tensors start out as sentinels too)
    grad = Carved([n]) if with_grad else None
    _call(LOSS_FN[kind], da.data_ptr(), db.data_ptr(), n, float(upstream), loss.ptr(), grad.ptr() if grad else None, partial.ptr())
    torch.cuda.synchronize()
    nb = min(1024, -(-n // 256))
    assert loss.intact() and partial.intact() and (grad is None or grad.intact()), f"{kind} n={n}: a sentinel changed"
    assert bool((partial.raw[partial.offs[0] + nb:] == SENT32).all()), f"{kind} n={n}: a partial sum beyond the grid was written"
    return loss.get()[0], grad


def _bce_model(x, y, upstream):
    """float32 format model of the BCE terms and gradient."""
    F = np.float32
    with np.errstate(over="ignore"):
        grad = (F(upstream) / F(x.size)) * (F(1) / (F(1) + np.exp(-x)) - y)
    return R.bce_terms(x, y), grad


def _check_bce(tag, x, y, upstream, loss, grad):
    """The BCE bounds: loss within accumulation bound + 4 E_term (E_term: largest per-term relative error of the float32 model),
    and within accumulation bound + 4 x the model's summed absolute term errors (the tighter statement where single terms
    underflow); gradient max-norm error within 4 x the model's."""
    n = x.size
    ref_loss, ref_grad = R.bce_logits(x, y, upstream)
    t64 = R.bce_terms(x.astype(np.float64), y.astype(np.float64))
    t32, g32 = _bce_model(x, y, upstream)
    assert t32.dtype == np.float32 and g32.dtype == np.float32
    e_term = float(np.max(np.abs(t32 - t64) / t64))
    acc = R.loss_accumulation_bound(n)
    err = abs(float(loss) - ref_loss) / ref_loss
    tight = acc + 4.0 * float(np.sum(np.abs(t32 - t64))) / float(np.sum(t64))
    g_err, g_model = R.max_rel(grad, ref_grad), R.max_rel(g32, ref_grad)
    print(f"train-err bce {tag} n={n} up={upstream}: loss {err:.2e} (bound {acc + 4 * e_term:.2e}, summed-term bound {tight:.2e}, "
          f"E_term {e_term:.2e}); grad {g_err:.2e} (model {g_model:.2e})")
    assert np.isfinite(loss) and np.isfinite(grad).all()
    assert err <= acc + 4.0 * e_term and err <= tight
    assert g_err <= 4.0 * g_model


@pytest.mark.parametrize("n", LOSS_N)
@pytest.mark.parametrize("kind", ["mse", "bce"])
def test_loss_and_gradient_against_float64(kind, n):
    a, b = _loss_inputs(kind, n)
    da, db = _dev(a), _dev(b)
    for up in UPSTREAMS:
        loss, grad = _run_loss(kind, da, db, up)
        g = grad.get()
        if kind == "bce":
            _check_bce("random", a, b, up, loss, g)
            continue
        ref_loss, ref_grad = R.mse(a, b, up)
        err, bound = abs(float(loss) - ref_loss) / ref_loss, R.loss_accumulation_bound(n)
        # gradient: upstream * 2 / n rounded once on the host, a - b rounded once, their product rounded once: (1 + 2^-24)^3 < 1 + 5 * 2^-24
        g_err = float(np.max(np.abs(g - ref_grad) / np.abs(ref_grad)))
        print(f"train-err mse n={n} up={up}: loss {err:.2e} (bound {bound:.2e}); grad {g_err:.2e} (bound {5 * U24:.2e})")
        assert err <= bound
        assert bool(np.all(np.abs(g - ref_grad) <= 5 * U24 * np.abs(ref_grad)))
    for up in (UPSTREAMS[0], UPSTREAMS[2]):       # grad == NULL: the same loss bits, and nothing written (asserted in _run_loss)
        with_grad, _ = _run_loss(kind, da, db, up)
        without, _ = _run_loss(kind, da, db, up, with_grad=False)
        assert with_grad.view(np.int32) == without.view(np.int32)


@pytest.mark.parametrize("kind", ["mse", "bce"])
def test_loss_counts_every_element_exactly_once(kind):
    """One non-zero term at index i of N1, everything else exactly zero: the loss is that term / n and the gradient is non-zero
    at i only.  An element skipped or visited twice by the grid-stride loop changes the loss by a factor (0 or 2) and leaves a
    sentinel NaN (or nothing) in the gradient -- which no tolerance on random inputs guarantees to see.
    MSE: a == b except a[i] - b[i] = 1: every operation is exact, the float64 mean is cast once: float32(1 / n) to 1 ulp.
    BCE: x = -200, y = 0 (term max(x, 0) - x y + log1p(exp(-200)) = 0 exactly, gradient 1 / (1 + Inf) = 0) except x[i] = 0
    (term log1pf(1), within 2 ulp of ln 2 on the device; the cast adds 1/2): float32(ln 2 / n) to 4 ulp."""
    n = R.N1
    if kind == "mse":
        base = hashed(13, (n,)).astype(np.float32)
        da, db = _dev(base), _dev(base)
        spike, want, ulps = (0.5, -0.5), np.float32(1.0 / n), 1
        want_g = np.float32(2.0) / np.float32(n)
    else:
        da, db = _dev(np.full(n, -200.0, np.float32)), _dev(np.zeros(n, np.float32))
        spike, want, ulps = (0.0, 0.0), np.float32(np.log(2.0) / n), 4
        want_g = (np.float32(1.0) / np.float32(n)) * np.float32(0.5)
    for i in R.SPIKES:
        keep = (float(da[i]), float(db[i]))
        da[i], db[i] = spike
        loss, grad = _run_loss(kind, da, db, 1.0)
        da[i], db[i] = keep
        g = grad.view()
        nz = torch.nonzero(g != 0).flatten().tolist()       # (a NaN left by a skipped element is != 0)
        assert nz == [i], f"{kind} spike at {i}: gradient non-zero at {nz[:8]}"
        assert float(g[i]) == float(want_g)
        d = abs(int(np.float32(loss).view(np.int32)) - int(want.view(np.int32)))
        assert d <= ulps, f"{kind} spike at {i}: loss {loss!r}, want {want!r} ({d} ulp)"


def test_bce_edge_logits():
    """x in {0, +-1e-4, +-20, +-88, +-104, +-200} with y in {0, 1, 0.3}: finite, and inside the bounds of the random case.
    expf(104) overflows inside the sigmoid: 1 / (1 + Inf) must be 0, not NaN; log1p(exp(-|x|)) underflows to 0."""
    xs = [0.0] + [s * v for v in (1e-4, 20.0, 88.0, 104.0, 200.0) for s in (1.0, -1.0)]
    x = np.array([v for v in xs for _ in range(3)], dtype=np.float32)
    y = np.array([0.0, 1.0, 0.3] * len(xs), dtype=np.float32)
    for up in UPSTREAMS:
        loss, grad = _run_loss("bce", _dev(x), _dev(y), up)
        _check_bce("edges", x, y, up, loss, grad.get())


# ================================================================================================ amax, loss scale, scale
def _amax(*tensors):
    """max|x| folded over device tensors into one zeroed cell -> its uint32 bits."""
    cell = Carved([1])
    cell.view().zero_()
    for t in tensors:
        _call("sos_amax_f32", t.data_ptr(), t.numel(), cell.ptr())
    torch.cuda.synchronize()
    assert cell.intact()
    return int(cell.get().view(np.uint32)[0])


def _bits(v):
    return int(np.float32(v).view(np.uint32))


@pytest.mark.parametrize("n", [1, 257, R.N1])
def test_amax_is_exact(n):
    x = (0.9 * hashed(21, (n,))).astype(np.float32)
    dx = _dev(x)
    assert _amax(dx) == _bits(np.max(np.abs(x)))
    zeros = torch.zeros(n, dtype=torch.float32, device="cuda")
    for i in [s for s in R.SPIKES if s < n]:
        keep = float(dx[i])
        dx[i] = -1.5                                        # the maximum, negative, at every trip / block edge
        assert _amax(dx) == _bits(1.5), i
        dx[i] = keep
        zeros[i] = -0.0                                     # -0 among zeros: |x| = +0
        assert _amax(zeros) == 0, i
        zeros[i] = 0.0
    # two tensors folded into one cell, in either order
    y = (3.0 * hashed(22, (300,))).astype(np.float32)
    dy = _dev(y)
    want = _bits(max(np.max(np.abs(x)), np.max(np.abs(y))))
    assert _amax(dx, dy) == want and _amax(dy, dx) == want
    # NaN elements are ignored (also a whole tensor of them), an Inf gives Inf
    for i in [s for s in R.SPIKES if s < n]:
        dx[i] = float("nan")
    rest = np.delete(x, [s for s in R.SPIKES if s < n])
    assert _amax(dx) == (_bits(np.max(np.abs(rest))) if rest.size else 0)
    assert _amax(torch.full((n,), float("nan"), device="cuda"), dy) == _bits(np.max(np.abs(y)))
    dx[n - 1] = float("-inf")
    assert _amax(dx) == 0x7F800000


def test_loss_scale_is_the_exact_power_of_two():
    """S = 2^floor(log2(target * back-off / amax)), both words, at every power-of-two edge of amax: 2^j, its 3 successors and 2
    predecessors, j in [-45, 45] (the edges of target 256), the same neighbourhoods of 100 * 2^j (the edges of target 100); amax 0,
    3.2e38 and Inf give 1.
    Just above an edge the float32 quotient is the float below a power of two, 2^k (1 - 2^-24) or 2^k (1 - 2^-23); its log2 is
    k - 1e-7, which a correctly rounded log2f returns as k: floor(log2f(q)) in correctly rounded float32 arithmetic disagrees with
    the exact rule in 191 of the 366 amax values 1-6 floats above 2^j.  Observed on MI355X: the kernel's floorf(log2f(q)) agrees
    with the exact rule in every case of this test (5 304 launches) -- the device's log2f does not round up to the integer.  This
    test is what holds the kernel to that."""
    vals = R.loss_scale_amax_values() + [v for j in range(-45, 46, 5) for v in R.neighbours(np.float32(100.0) * np.float32(2.0 ** j))]
    vals += [np.float32(0.0), np.float32(3.2e38), np.float32(np.inf)]
    amax = _dev(np.array(vals, dtype=np.float32))
    for target in (256.0, 100.0):
        for backoff in (None, 0.0, 0.5, 2.0 ** -20):
            guard = None if backoff is None else _dev(np.array([0.0, backoff, 0.0, 0.0, 0.0], dtype=np.float32))
            out = Carved([2 * len(vals)])
            for k in range(len(vals)):
                _call("sos_loss_scale", amax.data_ptr() + 4 * k, target, out.ptr() + 8 * k, guard.data_ptr() if guard is not None else None)
            torch.cuda.synchronize()
            assert out.intact()
            got = out.get().reshape(-1, 2)
            want = np.array([R.loss_scale(v, target, backoff) for v in vals], dtype=np.float32)
            bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
            assert bad.size == 0, (f"target {target} back-off {backoff}: {bad.size} of {len(vals)} differ, first "
                                   + ", ".join(f"amax {float(vals[k]).hex()} got {got[k].tolist()} want {want[k].tolist()}" for k in bad[:4]))


@pytest.mark.parametrize("n", [1, R.N2])
def test_scale_is_the_float32_product(n):
    x = hashed(23, (n,)).astype(np.float32)
    buf = Carved([n]).put(0, x)
    s = _dev(np.array([0.37], dtype=np.float32))
    _call("sos_scale_f32", buf.ptr(), n, s.data_ptr())
    torch.cuda.synchronize()
    assert buf.intact()
    assert np.array_equal(buf.get().view(np.uint32), (x * np.float32(0.37)).view(np.uint32))


# ================================================================================================================== guard
def _guard_state(words):
    st = Carved([5])
    st.view().copy_(torch.tensor([float(w) for w in words[:4]] + [0.0]))
    st.raw[st.offs[0] + 4] = int(words[4])
    return st


def _guard_words(st):
    torch.cuda.synchronize()
    assert st.intact()
    w = st.get()
    return [float(v) for v in w[:4]] + [int(w.view(np.uint32)[4])]


def test_guard_scan_finds_every_non_finite_word():
    n = R.N1
    g = _dev(hashed(31, (n,)).astype(np.float32))
    gi = g.view(torch.int32)
    st = _guard_state([0, 0, 0, 0, 0])
    for word in (0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001):
        for i in R.SPIKES:
            keep = int(gi[i])
            gi[i] = _i32(word)
            st.view().zero_()
            _call("sos_grad_guard", g.data_ptr(), n, st.ptr(), 1)
            assert _guard_words(st) == R.guard_finalize([0, 0, 0, 0, 0], True), (hex(word), i)
            gi[i] = keep
    # finite buffers: nothing found -- the plain one, and one of nothing but +-FLT_MAX, subnormals and +-0
    fmax = np.finfo(np.float32).max
    edge = np.array([fmax, -fmax, 1e-40, -1e-40, 0.0, -0.0], dtype=np.float32).view(np.uint32)
    edge = np.concatenate([edge, np.array([1, 0x807FFFFF], dtype=np.uint32)])
    tiled = _dev(np.resize(edge, n).view(np.float32))
    for buf in (g, tiled):
        st.view().zero_()
        _call("sos_grad_guard", buf.data_ptr(), n, st.ptr(), 1)
        assert _guard_words(st) == R.guard_finalize([0, 0, 0, 0, 0], False)


def test_guard_state_machine_step_by_step():
    """All five words after every finalize, against train_reference.guard_finalize: 22 overflows in a row (halved from `0 reads as
    1' to the floor 2^-20), 400 finite steps (a doubling at 200 and at 400, counter reset), growth stopping at 1 (the counter
    goes on counting), finalize = 0 (words 0-3 untouched, the flag kept for the finalizing call), the scratch word cleared."""
    n = 257
    good = torch.zeros(n, dtype=torch.float32, device="cuda")
    bad = good.clone()
    bad[n - 1] = float("inf")                               # in the second workgroup

    def run(st, buf, finalize=1):
        _call("sos_grad_guard", buf.data_ptr(), n, st.ptr(), finalize)
        return _guard_words(st)

    st, ref = _guard_state([0, 0, 0, 0, 0]), [0.0, 0.0, 0.0, 0.0, 0]
    for k in range(22):
        ref = R.guard_finalize(ref, True)
        assert run(st, bad) == ref, ("overflow", k)
    assert ref[1] == 2.0 ** -20 and ref[3] == 22.0
    for k in range(400):
        ref = R.guard_finalize(ref, False)
        assert run(st, good) == ref, ("finite", k)
    assert ref == [0.0, 2.0 ** -18, 0.0, 22.0, 0]
    st, ref = _guard_state([0, 0.25, 0, 5, 0]), [0.0, 0.25, 0.0, 5.0, 0]
    for k in range(650):
        ref = R.guard_finalize(ref, False)
        assert run(st, good) == ref, ("growth", k)
    assert ref == [0.0, 1.0, 250.0, 5.0, 0]
    # finalize = 0: only the scratch word moves; the finalizing call (over a finite buffer) sees the flag
    start = [0.0, 0.5, 7.0, 2.0, 0]
    st = _guard_state(start)
    got = run(st, bad, finalize=0)
    assert got[:4] == start[:4] and got[4] != 0
    assert run(st, good, finalize=1) == R.guard_finalize(start, True) == [1.0, 0.25, 0.0, 3.0, 0]
    st = _guard_state(start)
    assert run(st, good, finalize=0) == start
    assert run(st, good, finalize=1) == R.guard_finalize(start, False)
    # a scratch word left set is consumed and cleared
    st = _guard_state([0.0, 1.0, 3.0, 0.0, 1])
    assert run(st, good) == R.guard_finalize([0.0, 1.0, 3.0, 0.0, 1], False) == [1.0, 0.5, 0.0, 1.0, 0]


# =================================================================================================================== Adam
def _adam_single(p, g, m, v, step, wd, gs, skip=None, hyper=H):
    """sos_adam_step on copies -> (p, m, v) float32, sentinels checked."""
    n = p.size
    st = Carved([n, n, n]).put(0, p).put(1, m).put(2, v)
    dg = _dev(g)
    _call("sos_adam_step", st.ptr(0), dg.data_ptr(), st.ptr(1), st.ptr(2), n, hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"],
          wd, step, gs, skip.data_ptr() if skip is not None else None)
    torch.cuda.synchronize()
    assert st.intact(), "sos_adam_step wrote outside p / m / v"
    return st.get(0), st.get(1), st.get(2)


def _adam_multi(ps, gs_, ms, vs, step, wd, gs, skip=None, hyper=H, reverse=False, sent=None):
    """ONE sos_adam_multi_step over tensors carved from one buffer each (sentinels between them, a chunk of sentinels behind the
    last); the chunk table as sos_hip.h describes it: (tensor, chunk) for every chunk of every tensor."""
    sizes = [p.size for p in ps]
    P, G, M, V = (Carved(sizes, tail=R.ADAM_CHUNK, sent=sent) for _ in range(4))
    for i in range(len(ps)):
        P.put(i, ps[i]), G.put(i, gs_[i]), M.put(i, ms[i]), V.put(i, vs[i])
    g_before = G.raw.clone()
    rows = [[P.ptr(i), G.ptr(i), M.ptr(i), V.ptr(i), sizes[i]] for i in range(len(ps))]
    chunks = [[i, c] for i in range(len(ps)) for c in range(-(-sizes[i] // R.ADAM_CHUNK))]
    if reverse:
        chunks = chunks[::-1]
    tab = torch.tensor(rows, dtype=torch.int64, device="cuda")
    ch = torch.tensor(chunks, dtype=torch.int32, device="cuda")
    _call("sos_adam_multi_step", tab.data_ptr(), len(rows), ch.data_ptr(), len(chunks), hyper["lr"], hyper["b1"], hyper["b2"],
          hyper["eps"], wd, step, gs, skip.data_ptr() if skip is not None else None)
    torch.cuda.synchronize()
    assert P.intact() and M.intact() and V.intact(), "sos_adam_multi_step wrote outside a tensor"
    assert torch.equal(G.raw, g_before)
    return [(P.get(i), M.get(i), V.get(i)) for i in range(len(ps))]


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _check_adam(tag, got, p, g, m, v, step, wd, gs, skipped=0, p_scale=None):
    """m, v: max-norm relative error <= 8 * 2^-24 (at most 6 roundings each: g * grad_scale, + wd p, the two products, the sum --
    for v the square too).  Update: E <= 4 x the float32 model's E.  -> (E, E of the model)."""
    args = dict(wd=wd, step=step, grad_scale=gs, skipped=skipped, **H)
    ref, mod = R.adam_step(p, g, m, v, **args), R.adam_step_f32(p, g, m, v, **args)
    e, e_model = R.update_error(got[0], ref[0], p), R.update_error(mod[0], ref[0], p)
    e_m, e_v = R.max_rel(got[1], ref[1]), R.max_rel(got[2], ref[2])
    if p_scale is not None:
        assert e_model < R.ADAM_MODEL_E_MAX[p_scale], (tag, e_model)
    assert e_m <= 8 * U24 and e_v <= 8 * U24, (tag, e_m, e_v)
    assert e <= 4.0 * e_model, (tag, e, e_model)
    return e, e_model, e_m, e_v


@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_adam_one_step_against_float64(step):
    """sos_adam_step and sos_adam_multi_step from a given state, over |g| in {1, 1e-4, 1e-8} (at 1e-8 eps is as large as
    sqrt(v): its place in the formula shows), |p| in {1, 1e-3}, weight decay {0, 0.01}, grad_scale {1, 1/8, 1/3}."""
    n = 777
    worst = dict(e=0.0, ratio=0.0, m=0.0, v=0.0)
    for c in R.adam_grid():
        if c["step"] != step:
            continue
        p, g, m, v = R.adam_case(c["seed"], n, c["g_scale"], c["p_scale"], step == 1)
        one = _adam_single(p, g, m, v, step, c["wd"], c["grad_scale"])
        multi = _adam_multi([p], [g], [m], [v], step, c["wd"], c["grad_scale"])[0]
        assert _same_bits(one, multi), c
        e, e_model, e_m, e_v = _check_adam(c, one, p, g, m, v, step, c["wd"], c["grad_scale"], p_scale=c["p_scale"])
        worst = dict(e=max(worst["e"], e), ratio=max(worst["ratio"], e / e_model), m=max(worst["m"], e_m), v=max(worst["v"], e_v))
    print(f"train-err adam step={step}: worst E {worst['e']:.2e}, worst E / model E {worst['ratio']:.2f} (bound 4), "
          f"m {worst['m'] / U24:.2f} v {worst['v'] / U24:.2f} units of 2^-24 (bound 8)")


def test_adam_skipped_steps_move_the_bias_corrections():
    """skip = the guard state: [3] steps were skipped, so the corrections are taken at step - [3] applied updates (at least 1);
    [0] != 0 turns the launch into a no-op: p, m and v keep their bits."""
    n, wd, gs = 777, 0.01, 0.125
    p, g, m, v = R.adam_case(77, n, 1e-4, 1.0, False)
    for skipped, step in ((3, 10), (12, 10), (10, 10)):
        skip = _dev(np.array([0.0, 1.0, 0.0, float(skipped), 0.0], dtype=np.float32))
        one = _adam_single(p, g, m, v, step, wd, gs, skip=skip)
        multi = _adam_multi([p], [g], [m], [v], step, wd, gs, skip=skip)[0]
        assert _same_bits(one, multi)
        e, e_model, _, _ = _check_adam(("skipped", skipped), one, p, g, m, v, step, wd, gs, skipped=skipped, p_scale=1.0)
        # ... and the corrections of the attempt count lie at least 10 x outside the bound: the case can tell the two apart
        wrong = R.adam_step(p, g, m, v, wd=wd, step=step, grad_scale=gs, **H)
        right = R.adam_step(p, g, m, v, wd=wd, step=step, grad_scale=gs, skipped=skipped, **H)
        assert R.update_error(wrong[0], right[0], p) > 40.0 * e_model
        print(f"train-err adam skipped={skipped} step={step}: E {e:.2e} (model {e_model:.2e})")
    skip = _dev(np.array([1.0, 0.5, 0.0, 3.0, 0.0], dtype=np.float32))
    assert _same_bits(_adam_single(p, g, m, v, 10, wd, gs, skip=skip), (p, m, v))
    assert _same_bits(_adam_multi([p], [g], [m], [v], 10, wd, gs, skip=skip)[0], (p, m, v))


def test_adam_multi_tensor_chunk_edges():
    """One launch over tensors of 1, 255, 256, 257, 16383, 16384, 16385, 32768 and 32773 elements (SOS_ADAM_CHUNK = 16384): every
    tensor bit-identical to sos_adam_step on a copy and inside the bounds, every sentinel between the tensors intact -- a chunk's
    last workgroup stops at its tensor's end.  The chunk list in table order between signalling-NaN sentinels, and reversed
    between finite ones."""
    step, wd, gs = 10, 0.01, 1.0 / 3.0
    cases = [R.adam_case(500 + i, n, 1e-4, 1e-3, False) for i, n in enumerate(R.CHUNK_SIZES)]
    ps, gs_, ms, vs = (list(t) for t in zip(*cases))
    singles = [_adam_single(p, g, m, v, step, wd, gs) for p, g, m, v in cases]
    for reverse in (False, True):
        multi = _adam_multi(ps, gs_, ms, vs, step, wd, gs, reverse=reverse, sent=SENT32_FINITE if reverse else None)
        for i, n in enumerate(R.CHUNK_SIZES):
            assert _same_bits(multi[i], singles[i]), (n, reverse)
    for i, n in enumerate(R.CHUNK_SIZES):
        if n >= 255:        # (a bound relative to the largest of one or two elements says little; they are covered bit for bit)
            _check_adam(("chunks", n), singles[i], *cases[i], step, wd, gs)


def test_adam_step_past_the_grid_cap():
    """sos_adam_step at N2 = 524288 + 300: the 2048-block grid takes a second trip for the first 300 elements only."""
    step, wd, gs = 1000, 0.01, 0.125
    p, g, m, v = R.adam_case(600, R.N2, 1e-4, 1e-3, False)
    got = _adam_single(p, g, m, v, step, wd, gs)
    e, e_model, e_m, e_v = _check_adam("N2", got, p, g, m, v, step, wd, gs, p_scale=1e-3)
    print(f"train-err adam N2: E {e:.2e} (model {e_model:.2e}), m {e_m / U24:.2f} v {e_v / U24:.2f} units of 2^-24")


def test_fused_adam_chunk_table_over_three_steps():
    """agent.FusedAdam (its _table builds the device tables) on parameters of 1, 16384, 16385 and 40000 elements, weight decay
    0.01, grad_scale 0.5, three steps: the trajectory against adam_step iterated, E <= 4 x the iterated float32 model's.  (|g| ~ 1
    against |p| ~ 1e-3: three updates of ~1e-3 may carry p through zero, and 0.5 g + 0.01 p must not cancel.)"""
    from sos_amd.agent import FusedAdam
    sizes, wd, gs = [1, 16384, 16385, 40000], 0.01, 0.5
    p0 = [R.adam_case(700 + i, n, 1.0, 1e-3, True)[0] for i, n in enumerate(sizes)]
    params = [torch.nn.Parameter(_dev(p)) for p in p0]
    opt = FusedAdam(params, lr=H["lr"], betas=(H["b1"], H["b2"]), eps=H["eps"], weight_decay=wd)
    opt.grad_scale = gs
    ref = [(p.astype(np.float64), np.zeros(p.size), np.zeros(p.size)) for p in p0]
    mod = [(p, np.zeros_like(p), np.zeros_like(p)) for p in p0]
    for step in (1, 2, 3):
        for i, n in enumerate(sizes):
            g = R.adam_case(800 + 10 * step + i, n, 1.0, 1e-3, True)[1]
            params[i].grad = _dev(g)
            args = dict(wd=wd, step=step, grad_scale=gs, **H)
            ref[i] = R.adam_step(ref[i][0], g, ref[i][1], ref[i][2], **args)
            mod[i] = R.adam_step_f32(mod[i][0], g, mod[i][1], mod[i][2], **args)
        opt.step()
    torch.cuda.synchronize()
    cat = np.concatenate
    got = cat([p.detach().cpu().numpy() for p in params])
    e = R.update_error(got, cat([r[0] for r in ref]), cat(p0))
    e_model = R.update_error(cat([q[0] for q in mod]), cat([r[0] for r in ref]), cat(p0))
    print(f"train-err FusedAdam 3 steps: E {e:.2e} (model {e_model:.2e})")
    assert e_model < R.ADAM_MODEL_E_MAX[1e-3]
    assert e <= 4.0 * e_model


# ======================================================================================================== packed weights
PACK_N = (1, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 16384 + 1027)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_gather_pack_multi_bit_for_bit(mode):
    """Several entries in one launch, sizes around the 256-thread row, the 4-way unrolled 1024-element step and the 16384-element
    chunk; idx cycles through +address (the value), -address (its low part) and 0 (zero padding); the source elements are a
    permutation of one float tensor holding train_reference.pack_values.  Output bit-identical to train_reference.gather_pack,
    every sentinel between and behind the outputs intact.  (idx arrays lie in one buffer with zeros between and behind them.)"""
    import sos_amd
    sos_amd.set_precision(mode)
    try:
        vals = R.pack_values(mode)
        nv = vals.size
        assert nv % 3 != 0 and 3 * nv <= 16384              # every value meets every kind inside the large entries
        src = _dev(vals)
        rng = np.random.default_rng(9)
        perm = rng.permutation(nv)
        out = Carved(PACK_N, tail=R.ADAM_CHUNK, dtype=torch.int16)
        gap = 64
        idx_host = np.zeros(sum(n + gap for n in PACK_N) + R.ADAM_CHUNK, dtype=np.int64)
        rows, want, off = [], [], 0
        idx_dev = torch.zeros(idx_host.size, dtype=torch.int64, device="cuda")
        for e, n in enumerate(PACK_N):
            k = np.arange(n)
            which = perm[(k + 17 * e) % nv]
            kinds = 1 - (k + e) % 3                         # +1, 0, -1, ...
            idx_host[off:off + n] = kinds * (src.data_ptr() + 4 * which)
            rows.append([idx_dev.data_ptr() + 8 * off, out.ptr(e), n])
            want.append(R.gather_pack(vals[which], kinds, mode))
            off += n + gap
        idx_dev.copy_(torch.from_numpy(idx_host))
        chunks = [[e, c] for e, n in enumerate(PACK_N) for c in range(-(-n // R.ADAM_CHUNK))]
        tab = torch.tensor(rows, dtype=torch.int64, device="cuda")
        ch = torch.tensor(chunks, dtype=torch.int32, device="cuda")
        _call("sos_gather_pack_multi", tab.data_ptr(), len(rows), ch.data_ptr(), len(chunks))
        torch.cuda.synchronize()
        assert out.intact(), "sos_gather_pack_multi wrote outside an entry"
        for e, n in enumerate(PACK_N):
            got = out.get(e).view(np.uint16)
            bad = np.nonzero(got != want[e])[0]
            assert bad.size == 0, (mode, n, bad[:5], [hex(int(x)) for x in got[bad[:5]]], [hex(int(x)) for x in want[e][bad[:5]]])
    finally:
        sos_amd.set_precision("bf16")
