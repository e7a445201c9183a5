"""TEST INFRASTRUCTURE: float64 / exact-integer references of the training-step kernels (csrc/train.hip), written from the
C ABI's documentation (include/sos_hip.h) and the torch semantics it cites -- nn.MSELoss, nn.BCEWithLogitsLoss,
torch.optim.Adam (amsgrad off), torch.cuda.amp.GradScaler's skipped steps, Tensor.to(bfloat16 / float16).  numpy only.
tests/test_train_reference.py pins this file against torch on the CPU; tests/test_gpu_train_kernels.py compares the kernels
with it.

`adam_step_f32` is a FORMAT MODEL, not a reference: the same formula evaluated in float32.  It is used only to size bounds
(`the kernel adds nothing beyond its number format'), as tests/storage_model.py is for the 16-bit storage types."""
import numpy as np

ADAM_CHUNK = 16384          # SOS_ADAM_CHUNK
GUARD_GROWTH = 200          # SOS_GUARD_GROWTH
GUARD_FLOOR = 2.0 ** -20
LOSS_BLOCKS = 1024          # grid cap of the loss / amax / guard kernels (256 threads each)
N1 = 2 * LOSS_BLOCKS * 256 + 257        # some threads of a capped 1024-block grid take 3 trips, some 2
N2 = 2048 * 256 + 300                   # past the 2048-block cap of sos_adam_step / sos_scale_f32
CHUNK_SIZES = (1, 255, 256, 257, 16383, 16384, 16385, 32768, 32773)
SPIKES = (0, 255, 256, N1 - 1, 262143, 262144, 524287, 524288)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(x):
    """A scalar as the C ABI receives it (float), back in float64."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------- losses
def mse(a, b, upstream=1.0):
    """nn.MSELoss() (mean) and upstream * d loss / d a."""
    a, b = _f64(a).ravel(), _f64(b).ravel()
    d = a - b
    return float(np.mean(d * d)), f32(upstream) * 2.0 * d / d.size


def sigmoid(x):
    x = _f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_terms(x, y):
    """Per-element nn.BCEWithLogitsLoss terms, max(x, 0) - x y + log1p(exp(-|x|)), in the dtype of the inputs."""
    with np.errstate(under="ignore"):
        return np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))


def bce_logits(x, y, upstream=1.0):
    """nn.BCEWithLogitsLoss() (mean) and upstream * d loss / d x."""
    x, y = _f64(x).ravel(), _f64(y).ravel()
    return float(np.mean(bce_terms(x, y))), f32(upstream) * (sigmoid(x) - y) / x.size


def loss_accumulation_bound(n):
    """Relative bound of the two-stage sum of n non-negative float32 terms: each of the min(1024, ceil(n / 256)) * 256 threads
    adds its k terms one by one (k roundings; MSE's fused multiply-add rounds d*d + acc once, the rounding of d = a - b enters the
    term twice), a 256-wide tree follows (8 levels), the block sums are added in float64 and the mean is cast (1):
    (k + 2 + 8 + 1) * 2^-24."""
    blocks = min(LOSS_BLOCKS, -(-n // 256))
    k = -(-n // (256 * blocks))
    return (k + 11) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ Adam
def _bias_steps(step, skipped):
    return max(int(step) - int(skipped), 1)


def adam_step(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, skipped=0):
    """One torch.optim.Adam (amsgrad=False) update in float64 -> (p, m, v).  The gradient is grad_scale * g, L2 weight decay is
    added to it; `step` counts attempts, `skipped` of which were dropped by the overflow guard: the bias corrections are taken at
    the number of applied updates (GradScaler semantics), at least 1."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    lr, b1, b2, eps, wd, gs = (f32(h) for h in (lr, b1, b2, eps, wd, grad_scale))
    t = _bias_steps(step, skipped)
    g = g * gs + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def adam_step_f32(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, skipped=0):
    """The formula of adam_step with every operation rounded to float32 (format model, see the module docstring)."""
    F = np.float32
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (F(h) for h in (lr, b1, b2, eps, wd, grad_scale))
    t = F(_bias_steps(step, skipped))
    one = F(1)
    g = g * gs + wd * p
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    bc1, bc2 = one - b1 ** t, one - b2 ** t
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    out = p - (lr / bc1) * (m / denom)
    assert out.dtype == F and m.dtype == F and v.dtype == F
    return out, m, v


def update_error(p_got, p_ref, p0):
    """E of an update: the error of the CHANGE of p, relative to the largest change (p itself hides a 5e-4 relative error of
    a 1e-3 |p| update behind its own size)."""
    p_got, p_ref, p0 = _f64(p_got), _f64(p_ref), _f64(p0)
    return float(np.max(np.abs((p_got - p0) - (p_ref - p0))) / np.max(np.abs(p_ref - p0)))


def max_rel(got, ref):
    got, ref = _f64(got), _f64(ref)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def adam_case(seed, n, g_scale, p_scale, first):
    """Inputs of one Adam step as float32 arrays (p, g, m, v): |p| in [p_scale / 4, p_scale], |g| in [g_scale / 4, g_scale] (so
    v stays a normal number down to g_scale 1e-8), m ~ g_scale, v ~ g_scale^2; `first`: the state of step 1 (m = v = 0).  g has the sign
    of p: grad_scale * g + weight_decay * p must not cancel, or the update of an element whose sum lands near eps amplifies the
    sum's rounding error 1e4-fold and the format model stops being a yardstick (test_train_reference.py checks that it is one)."""
    rng = np.random.default_rng(seed)
    # |p| in [p_scale / 4, p_scale]: at g_scale 1e-8 with grad_scale 1/8 the largest update is 1e-4, and p's own grid (2^-25 |p|)
    # has to stay well below it
    p = (p_scale * rng.choice([-1.0, 1.0], n) * (0.25 + 0.75 * rng.random(n))).astype(np.float32)
    g = (g_scale * np.where(p < 0, -1.0, 1.0) * (0.25 + 0.75 * rng.random(n))).astype(np.float32)
    if first:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m = (g_scale * 0.5 * rng.standard_normal(n)).astype(np.float32)
    v = (g_scale * g_scale * (0.1 + rng.random(n))).astype(np.float32)
    return p, g, m, v


ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_G_SCALES = (1.0, 1e-4, 1e-8)
ADAM_P_SCALES = (1.0, 1e-3)
ADAM_WD = (0.0, 0.01)
ADAM_GRAD_SCALES = (1.0, 0.125, 1.0 / 3.0)
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
# the format model's own E has to stay below this for a case to be a usable yardstick: at |p| ~ 1 the update (~1e-3) is rounded
# to p's grid (2^-24 / 1e-3 = 6e-5); at |p| ~ 1e-3 only the formula's roundings and the float32 bias corrections remain
ADAM_MODEL_E_MAX = {1.0: 1e-3, 1e-3: 1e-5}


def adam_grid():
    """Every (step, g_scale, p_scale, wd, grad_scale) of the one-step tests, with a seed."""
    k = 0
    for step in ADAM_STEPS:
        for gsc in ADAM_G_SCALES:
            for psc in ADAM_P_SCALES:
                for wd in ADAM_WD:
                    for gs in ADAM_GRAD_SCALES:
                        k += 1
                        yield dict(seed=1000 + k, step=step, g_scale=gsc, p_scale=psc, wd=wd, grad_scale=gs)


# ------------------------------------------------------------------------------------------------------------ loss scale
def loss_scale(amax, target, backoff=None):
    """sos_loss_scale by the exact integer rule -> (S, 1 / S).  S = 2^e, e = floor(log2(T / amax)) clamped to [-40, 40], with
    T = target * backoff (a back-off <= 0 or None reads as 1): T = mt 2^et and amax = ma 2^ea with mantissas in [0.5, 1), so
    T / amax = (mt / ma) 2^(et - ea) with mt / ma in (0.5, 2) and e = et - ea - (mt < ma).  S = 1 when amax is 0, NaN or >= 3e38."""
    T = np.float32(target)
    if backoff is not None and np.float32(backoff) > 0:
        T = np.float32(T * np.float32(backoff))
    a = np.float32(amax)
    if not (a > 0) or not (a < np.float32(3.0e38)):
        return 1.0, 1.0
    mt, et = np.frexp(np.float64(T))
    ma, ea = np.frexp(np.float64(a))
    e = int(et) - int(ea) - (1 if mt < ma else 0)
    e = max(-40, min(40, e))
    return 2.0 ** e, 2.0 ** -e


def neighbours(x, up=3, down=2):
    """x as float32, its `up` successors and `down` predecessors."""
    x = np.float32(x)
    out, lo, hi = [x], x, x
    for _ in range(up):
        hi = np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
        out.append(hi)
    for _ in range(down):
        lo = np.nextafter(lo, np.float32(0), dtype=np.float32)
        out.append(lo)
    return out


def loss_scale_amax_values():
    """Every 2^j, j in [-45, 45], with its 3 float32 successors and 2 predecessors: the edges of the floor."""
    return [v for j in range(-45, 46) for v in neighbours(2.0 ** j)]


# ----------------------------------------------------------------------------------------------------------------- guard
def is_bad(bits):
    """Inf or NaN by the bit pattern: exponent all ones."""
    bits = np.asarray(bits).astype(np.uint32)
    return (bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)


def guard_finalize(state, bad=False):
    """The guard's state machine (sos_hip.h): state = [found, back-off, finite steps since the back-off changed, steps skipped,
    scratch flag word]; `bad`: the buffers scanned since the last finalize held an Inf / NaN (a set scratch word counts).  A
    back-off <= 0 reads as 1.  Overflow: found, one more skipped step, counter reset, back-off halved down to 2^-20.  Finite:
    not found, counter + 1, and once it reaches SOS_GUARD_GROWTH while the back-off is below 1 the back-off doubles (at most 1)
    and the counter restarts.  The scratch word is cleared."""
    found, b, fin, skipped, raw = state
    bad = bool(bad) or int(raw) != 0
    b = float(b) if b > 0 else 1.0
    if bad:
        found, skipped, fin, b = 1.0, skipped + 1.0, 0.0, max(0.5 * b, GUARD_FLOOR)
    else:
        found, fin = 0.0, fin + 1.0
        if fin >= GUARD_GROWTH and b < 1.0:
            b, fin = min(1.0, 2.0 * b), 0.0
    return [found, b, fin, skipped, 0]


# ------------------------------------------------------------------------------------------------------- packed weights
def _to_bf16_bits(u):
    """float32 bit patterns (finite or Inf) -> bfloat16 bit patterns, round to nearest even."""
    u = u.astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _to_half_bits(u):
    """float32 bit patterns (finite or Inf) -> IEEE half bit patterns, round to nearest even, in integers."""
    u = u.astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7FFFFFFF
    # normal halves: re-bias the exponent (127 - 15 = 112), add half an ulp of the 13 dropped bits (ties to even); a carry runs
    # into the exponent as it must; anything at or past 2^16 - 2^4 becomes Inf
    normal = np.minimum((a - (112 << 23) + 0xFFF + ((a >> 13) & 1)) >> 13, 0x7C00)
    # below 2^-14: the value in units of 2^-24 is the 24-bit significand shifted right by 126 - exponent
    e = a >> 23
    sig = np.where(e > 0, (a & 0x7FFFFF) | 0x800000, 0)
    sh = np.clip(126 - e, 1, 25)                    # (>= 25 places: less than half a unit, 0)
    q, rem, half = sig >> sh, sig & ((1 << sh) - 1), 1 << (sh - 1)
    sub = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    return (sign | np.where(a >= (113 << 23), normal, sub)).astype(np.uint16)


def _widen(h, dtype):
    if dtype == "bf16":
        return (h.astype(np.uint32) << 16).view(np.float32)
    return h.view(np.float16).astype(np.float32)


def to_storage_bits(x, dtype):
    """float32 values -> 16-bit storage bit patterns ('bf16' / 'fp16')."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert not np.isnan(x).any()
    return (_to_bf16_bits if dtype == "bf16" else _to_half_bits)(x.view(np.uint32))


def gather_pack(src, idx_kinds, dtype):
    """sos_gather_pack_multi's output for gathered float32 values `src` (finite): kind > 0 -> hi = the value rounded to the
    storage type; kind < 0 -> the low part, (v - float(hi)) rounded; kind 0 -> +0.  uint16 bit patterns."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    kinds = np.asarray(idx_kinds)
    assert np.isfinite(src).all() and kinds.shape == src.shape
    hi = to_storage_bits(src, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        rest = (src - _widen(hi, dtype)).astype(np.float32)         # exact; -+Inf where hi overflowed
    lo = to_storage_bits(rest, dtype)
    return np.where(kinds > 0, hi, np.where(kinds < 0, lo, np.uint16(0))).astype(np.uint16)


def pack_values(dtype, n_random=3000, seed=7):
    """The finite float32 values the packing is checked on: normals, exact round-to-even ties of the format (both parities of
    the kept bit, both signs, normal and subnormal halves), +-0, half subnormals, the largest halves and what lies past them,
    values next to FLT_MAX (which round to Inf in bfloat16)."""
    rng = np.random.default_rng(seed)
    vals = [rng.standard_normal(n_random).astype(np.float32), (1e-3 * rng.standard_normal(200)).astype(np.float32)]
    drop = 16 if dtype == "bf16" else 13
    ties = []
    for base in (0x3F800000, 0x3F810000, 0x40490000, 0x3A000000, 0x47000000):
        keep = base & ~((1 << drop) - 1)
        for odd in (0, 1):
            t = keep | (odd << drop) | (1 << (drop - 1))
            ties += [t, t | 0x80000000, t + 1, t - 1]
    vals.append(np.array(ties, dtype=np.uint32).view(np.float32))
    vals.append(np.array([0.0, -0.0, 1e-6, -1e-6, 6e-8, -6e-8, 2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -14,
                          2.0 ** -14 - 2.0 ** -25, 1e-30, -1e-30], dtype=np.float32))
    if dtype == "fp16":
        vals.append(np.array([65504.0, 65519.0, 65520.0, 70000.0, -65504.0, -65519.0, -65520.0, -70000.0], dtype=np.float32))
    else:
        fmax = np.float32(np.finfo(np.float32).max)
        vals.append(np.array([fmax, -fmax, np.nextafter(fmax, np.float32(0)), 3.3895313e38, 3.3961775e38, -3.3961775e38, 65504.0,
                              65520.0, 70000.0], dtype=np.float32))
    out = np.concatenate(vals)
    assert np.isfinite(out).all()
    return out
