"""The streaming resampler's rule on the CPU: the float64 restatement (tests/stream_resample_reference.py) reproduces
oracle.wave_io.resample exactly whatever the chunking, and the library's host-only sos_stream_resample_ready counts the final
outputs and the retained samples exactly as the restatement's literal running sum does."""
import ctypes as C

import numpy as np
import pytest

import stream_resample_reference as SR
from oracle import wave_io as owio

_rules = {}


def rule(pair):
    if pair not in _rules:
        _rules[pair] = SR.Rule(*pair)
    return _rules[pair]


def _ids(pair):
    return "%d-%d" % pair


def _chunkings(n, R, seed):
    """All at once; the named sizes in turn, repeated; random sizes up to 3 R (zeros among them)."""
    named, fixed, left = [1, 7, 0, R, R + 1, 2 * R + 3, 1000, 13], [], n
    while left:
        c = min(named[len(fixed) % len(named)], left)
        fixed.append(c)
        left -= c
    rng, rand, left = np.random.default_rng(seed), [], n
    while left:
        c = min(int(rng.integers(0, 3 * R + 1)), left)
        rand.append(c)
        left -= c
    return {"at once": [n], "named": fixed, "random": rand + [0]}


@pytest.mark.parametrize("pair", SR.RATE_PAIRS, ids=_ids)
def test_chunked_reference_is_the_whole_signal_exactly(pair):
    r = rule(pair)
    assert r.R == {44100: 202, 48000: 219, 16000: 73, 8000: 64, 14000: 64}[pair[0]]
    rng = np.random.default_rng(pair[0] + pair[1])
    for n in (1, 2 * r.R + 5, 9001):
        x = rng.standard_normal(n)
        whole = {fix: owio.resample(x, *pair, fix=fix) for fix in (True, False)}
        if int(n * r.ratio) < 1:
            with pytest.raises(ValueError, match="too small to resample"):
                r.stream(x, [n])
            continue
        # the ranged restatement is resample_f itself
        assert np.array_equal(r.outputs(x, n, 0, int(n * r.ratio))[0], owio.resample_f(x, r.ratio, r.win, r.num_table))
        for name, sizes in _chunkings(n, r.R, n).items():
            for fix in (True, False):
                pieces, most = r.stream(x, sizes, fix=fix)        # asserts finality, t < int(n_total * ratio), the pending bound
                assert len(pieces) == len(sizes) + 1 and most <= r.PENDING_BOUND
                assert np.array_equal(np.concatenate(pieces), whole[fix]), (pair, n, name, fix)
                if n == 9001:           # the bound is not loose: n(T) < n_recv - R + ceil(1 / ratio), so a long stream comes that close
                    assert most >= r.PENDING_BOUND + 1 - int(np.ceil(1 / r.ratio))


def _ready(h, r, n_recv):
    t, b = C.c_int64(-1), C.c_int64(-1)
    assert h.sos_stream_resample_ready(r.ratio, r.nwin, r.num_table, int(n_recv), C.byref(t), C.byref(b)) == 0, h.sos_last_error()
    return t.value, b.value


@pytest.mark.parametrize("pair", SR.RATE_PAIRS, ids=_ids)
def test_host_ready_is_the_reference_count(pair):
    from sos_amd import _lib
    h, r = _lib.lib(), rule(pair)
    rng = np.random.default_rng(pair[0])
    top = 2 ** 20 + int(2 ** 20 * pair[0] / pair[1])              # the outputs cross several binades of the register
    far = np.sort(rng.integers(3001, top, size=200)).tolist() + [top]
    last = (0, 0)
    for n_recv in list(range(3001)) + far:
        got = _ready(h, r, n_recv)
        assert got == r.ready(n_recv), (pair, n_recv)
        assert got[0] >= last[0] and got[1] >= last[1] and n_recv - got[1] <= r.PENDING_BOUND      # monotone, bounded
        last = got
    assert last[0] > 2 ** 18


def test_host_ready_refuses_bad_arguments():
    from sos_amd import _lib
    h = _lib.lib()
    t, b = C.c_int64(0), C.c_int64(0)
    good = dict(ratio=14000 / 48000, nwin=32769, num_table=512, n_recv=1000)
    for bad, told in ((dict(ratio=0.0), "ratio=0"), (dict(ratio=-1.0), "ratio=-1"), (dict(nwin=0), "nwin=0"),
                      (dict(ratio=1e-3), "too small for a 512-point table"), (dict(n_recv=-1), "-1 samples")):
        a = dict(good, **bad)
        assert h.sos_stream_resample_ready(a["ratio"], a["nwin"], a["num_table"], a["n_recv"], C.byref(t), C.byref(b)) == -22
        msg = h.sos_last_error().decode()
        assert msg.startswith("sos_stream_resample_ready:") and told in msg, msg
    assert h.sos_stream_resample_ready(good["ratio"], 32769, 512, 1000, None, C.byref(b)) == -22
    assert h.sos_stream_resample_ready(good["ratio"], 32769, 512, 1000, C.byref(t), C.byref(b)) == 0 and t.value > 0
