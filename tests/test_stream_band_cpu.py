"""The streaming band merge's rule on the CPU: the float64 restatement (tests/stream_band_reference.py) reproduces
band_reference's result for the whole signals exactly, whatever the chunking and however far the networks' output trails, within
its stated pending bounds; and the library's host-only sos_stream_band_ready counts the final outputs and the retained samples
and frames exactly as the restatement does."""
import ctypes as C

import numpy as np
import pytest

import stream_band_reference as SB
from test_stream_resample_cpu import _chunkings

HOP, LOW = 158, 14000
RATES = [48000, 44100]
SMOOTH = [0, 2, 16]
LEAD = 65                       # a trails what x gives by this many samples until the last step, as an input resampler's would
N = 12007                       # native samples: 23 (48 kHz) / 25 (44.1 kHz) frames of a, more than K = 16

_rules, _signals = {}, {}


def rule(rate, K):
    if (rate, K) not in _rules:
        _rules[rate, K] = SB.Rule(LOW, rate, HOP, K)
    return _rules[rate, K]


def signals(rate):
    if rate not in _signals:
        rng = np.random.default_rng(rate)
        x = rng.standard_normal(N)
        m = -(-N * LOW // rate)
        a = rng.standard_normal(m)
        a[5 * HOP:6 * HOP + 7] = 0.0                                  # a frame with E_a == 0
        env = 0.75 + 0.75 * np.sin(np.arange(m) / 300.0)             # 0 .. 1.5: r reaches 0, the inside of (0, 1) and the clip at 1
        b = (a * np.maximum(env, 0.0))[:HOP * (m // HOP)]
        _signals[rate] = (x, a, b)
    return _signals[rate]


def _steps(rate, sizes, lag):
    """The steps (c_x, c_a, c_b) of x fed in chunks of `sizes`: a follows x LEAD samples behind, b follows a as `lag` says; a last
    step without x brings the rest of a and b.  -> (steps, the largest m_x - m_b after a step)."""
    x, a, b = signals(rate)
    m, mp = len(a), len(b)
    n_x = m_a = m_b = worst = 0
    steps = []
    for c in list(sizes) + [None]:
        if c is None:
            new_a, new_b = m, mp
        else:
            n_x += c
            new_a = max(-(-n_x * LOW // rate) - LEAD, 0)
            new_b = {"behind": min(new_a, mp), "bursts": min(10 * HOP * (new_a // (10 * HOP)), mp), "last": 0}[lag]
        steps.append((c or 0, new_a - m_a, new_b - m_b))
        m_a, m_b = new_a, new_b
        worst = max(worst, -(-n_x * LOW // rate) - m_b)
    return steps, worst


@pytest.mark.parametrize("lag", ["behind", "bursts", "last"])
@pytest.mark.parametrize("K", [None] + SMOOTH, ids=lambda k: "keep" if k is None else "K%d" % k)
@pytest.mark.parametrize("rate", RATES)
def test_streamed_reference_is_the_whole_signal_exactly(rate, K, lag):
    r = rule(rate, K)
    x, a, b = signals(rate)
    want = SB.whole(r, x, a, b)
    assert len(want) == N
    for name, sizes in _chunkings(N, r.R, N).items():
        steps, worst = _steps(rate, sizes, lag)
        assert worst <= {"behind": LEAD + HOP, "bursts": LEAD + 11 * HOP, "last": len(a)}[lag]
        pieces, most = r.stream(x, a, b, steps, worst)               # asserts finality and the pending bounds at every step
        got = np.concatenate(pieces)
        assert len(pieces) == len(steps) + 1 and got.shape == (N,)
        assert np.array_equal(got, want), (rate, K, lag, name, int(np.argmax(got != want)))
        bound = r.bounds(worst)
        assert all(most[k] <= bound[k] for k in bound)
        if lag != "last":                                              # something is final before the close
            assert sum(len(p) for p in pieces[:-1]) > 0


def _ready(h, r, m_b, n_x):
    out = [C.c_int64(-1) for _ in range(5)]
    rc = h.sos_stream_band_ready(r.rho, r.up.nwin, r.up.num_table, r.hop, -1 if r.K is None else r.K, int(m_b), int(n_x),
                                 *[C.byref(v) for v in out])
    assert rc == 0, h.sos_last_error()
    return tuple(v.value for v in out)


@pytest.mark.parametrize("K", [None] + SMOOTH, ids=lambda k: "keep" if k is None else "K%d" % k)
@pytest.mark.parametrize("rate", RATES)
def test_host_ready_is_the_reference_count(rate, K):
    from sos_amd import _lib
    h, r = _lib.lib(), rule(rate, K)
    rng = np.random.default_rng(rate)
    far = np.sort(rng.integers(3001, 2 ** 20, size=200)).tolist() + [2 ** 20]
    last = (0,) * 5
    for m_b in list(range(3001)) + far:
        n_far = int((m_b + 70) * r.rho) + 5                           # x is never what holds an output back
        got = _ready(h, r, m_b, n_far)
        assert got == r.ready(m_b, n_far), (rate, K, m_b)
        assert all(g >= p for g, p in zip(got, last)), (m_b, got, last)      # monotone in m_b
        last = got
        for n_x in {0, got[0] // 2, max(got[0] - 1, 0), got[0], got[0] + 1}:      # x holds it back, or just does not
            assert _ready(h, r, m_b, n_x) == r.ready(m_b, n_x), (rate, K, m_b, n_x)
            assert _ready(h, r, m_b, n_x)[0] == min(n_x, got[0])
    assert last[0] > 2 ** 21


def test_host_ready_refuses_bad_arguments():
    from sos_amd import _lib
    h = _lib.lib()
    out = [C.c_int64(0) for _ in range(5)]
    refs = [C.byref(v) for v in out]
    good = dict(ratio=48000 / 14000, nwin=32769, num_table=512, hop=158, smooth=2, m_b=1000, n_x=4000)

    def call(a, refs=refs):
        return h.sos_stream_band_ready(a["ratio"], a["nwin"], a["num_table"], a["hop"], a["smooth"], a["m_b"], a["n_x"], *refs)

    for bad, told in ((dict(ratio=1.0), "ratio=1"), (dict(ratio=14000 / 48000), "above 1"), (dict(ratio=-1.0), "ratio=-1"),
                      (dict(nwin=0), "nwin=0"), (dict(num_table=0), "num_table=0"), (dict(nwin=100), "a wing of at least one sample"),
                      (dict(hop=0), "hop=0"), (dict(smooth=17), "smooth=17"), (dict(m_b=-1), "-1 low-rate"),
                      (dict(n_x=-5), "-5 native"), (dict(m_b=2 ** 52 + 1), "low-rate")):
        assert call(dict(good, **bad)) == -22, bad
        msg = h.sos_last_error().decode()
        assert msg.startswith("sos_stream_band_ready:") and told in msg, msg
    for k in range(5):
        assert call(good, refs[:k] + [None] + refs[k + 1:]) == -22
        assert h.sos_last_error().decode() == "sos_stream_band_ready: null pointer"
    assert call(good) == 0 and out[0].value > 0
    assert call(dict(good, smooth=-1)) == 0 and out[4].value == 0


def test_launch_entry_points_refuse_bad_rows_on_the_host():
    """sos_stream_band_merge_f32 / sos_stream_band_ratio_f64 check every HOST row before any HIP call: over dummy (never
    dereferenced) pointers, without a GPU, a bad row is SOS_EINVAL and is named."""
    from sos_amd import _lib
    h = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    cap, rcap, ratio = 8000, 60, 48000 / 14000

    def merge(rows, smooth=2, slots=3, nwin=32769, ring=p, **kw):
        tab = np.asarray(rows, dtype=np.int64)
        rc = h.sos_stream_band_merge_f32(ring, slots, kw.get("cap", cap), p, kw.get("rcap", rcap), p, tab.ctypes.data, len(rows),
                                         kw.get("ratio", ratio), p, nwin, 512, kw.get("hop", HOP), smooth, p, 64, None)
        return rc, h.sos_last_error().decode()

    def ratio_rows(rows, slots=3, **kw):
        tab = np.asarray(rows, dtype=np.int64)
        rc = h.sos_stream_band_ratio_f64(p, slots, kw.get("cap", cap), p, tab.ctypes.data, len(rows), kw.get("hop", HOP), p,
                                         kw.get("rcap", rcap), None)
        return rc, h.sos_last_error().decode()

    # merge rows {slot, t_lo, t_hi, n_x, n_a, n_b, v_b, J, r_hi, output offset}
    ok = [0, 0, 10, 2000, 500, 400, 10, -1, 3, 0]
    for rows, told in (([ok, [3, 0, 10, 2000, 500, 400, 10, -1, 3, 10]], "row 1 names a slot outside the slots"),
                       ([[0, 11, 10, 2000, 500, 400, 10, -1, 3, 0]], "row 0 has a range that is none"),
                       ([[0, 0, 10, 2000, 400, 500, 10, -1, 3, 0]], "row 0 has counts that do not fit"),
                       ([[0, 0, 10, 2000, 500, 400, 1372, -1, 3, 0]], "row 0 has counts that do not fit"),
                       ([[0, 0, 10, 2000, 500, 400, 10, -1, 3, 55]], "row 0 writes outside the output buffer"),
                       ([ok, [1, 0, 10, 9, 500, 400, 10, -1, 3, 10]], "row 1 reads native samples its ring does not hold"),
                       ([[0, 0, 10, cap + 1, 500, 400, 10, -1, 3, 0]], "row 0 reads native samples its ring does not hold"),
                       ([[0, 0, 10, 2000, cap + 1, 400, 10, -1, 3, 0]], "row 0 reads samples of a or b their rings do not hold"),
                       ([[0, 0, 10, 2000, 2, 2, 6, -1, 3, 0]], "row 0 reads samples of a or b their rings do not hold"),
                       ([[0, 0, 10, 2000, 500, 400, 10, -1, 2, 0]], "row 0 reads frames of r its ring of frames does not hold"),
                       ([[0, 0, 10, 2000, 500, 400, 10, 3, 4, 0]], "row 0 reads frames of r its ring of frames does not hold"),
                       ([[0, 0, 10, 2000, 500, 400, 10, 4, 3, 0]], "row 0 reads frames of r its ring of frames does not hold"),
                       ([[0, 0, 10, 2000, 500, 400, 10, -1, rcap + 1, 0]], "row 0 reads frames of r its ring of frames does not hold"),
                       ([ok, [1, 0, 10, 2000, 500, 400, 10, -1, 3, 10], [0, 10, 20, 2000, 500, 400, 20, -1, 3, 20]],
                        "row 2 names slot 0, which an earlier row")):
        rc, msg = merge(rows)
        assert rc == -22 and msg.startswith("sos_stream_band_merge_f32:") and told in msg, (rows, rc, msg)
    # every row above is refused before a launch, and an empty one asks for none: nothing here may reach a device
    assert merge([[0, 5, 5, 2000, 500, 400, 5, -1, 0, 0]], smooth=-1) == (0, msg)
    for kw, told in ((dict(slots=0), "1 .. 21845 slots"), (dict(slots=21846), "1 .. 21845 slots"), (dict(cap=0), "rings of 0 samples"),
                     (dict(hop=0), "hop=0"), (dict(ratio=1.0), "ratio=1"), (dict(smooth=17), "smooth=17"), (dict(rcap=0), "a ring of 0 frames"),
                     (dict(nwin=50000), "must fit the 160 KB LDS"), (dict(ring=None), "null pointer")):
        rc, msg = merge([ok], **kw)
        assert rc == -22 and told in msg, (kw, rc, msg)
    # ratio rows {slot, j_lo, j_hi, m_a, m_b}
    for rows, told in (([[3, 0, 1, 500, 400]], "row 0 names a slot outside the slots"),
                       ([[0, 2, 1, 500, 400]], "row 0 has a range that is none"),
                       ([[0, 0, 5, 500, 400]], "row 0 has a range that is none, or frames"),
                       ([[0, 0, rcap + 1, 20000, 400]], "row 0 has a range that is none, or frames"),
                       ([[0, 0, 1, 400, 500]], "row 0 has counts that do not fit"),
                       ([[0, 0, 1, cap + 1, 400]], "row 0 reads samples of a or b their rings do not hold"),
                       ([[0, 0, 1, 500, 400], [0, 1, 2, 500, 400]], "row 1 names slot 0, which an earlier row")):
        rc, msg = ratio_rows(rows)
        assert rc == -22 and msg.startswith("sos_stream_band_ratio_f64:") and told in msg, (rows, rc, msg)
    assert ratio_rows([[0, 0, 0, 500, 400], [1, 3, 3, 500, 400]]) == (0, msg)         # nothing to do: no launch, the error text stays
    from sos_amd import _lib as L
    assert all(name in L.SIGNATURES for name in ("sos_stream_band_ready", "sos_stream_band_ratio_f64", "sos_stream_band_merge_f32"))
