"""audio_io.StreamBandMerger (csrc/stream_band.hip): live streams x, a, b fed in chunks give resample_merge_batch_device's result
for the whole signals, bit for bit, under 'keep' and under 'follow' with band_gains_batch_device's gains -- whatever the chunking
and however far b trails.  No networks: a = resample_device(x), b = a times an envelope."""
import warnings

import numpy as np
import pytest
import torch

import band_reference as B

pytestmark = pytest.mark.gpu
SR, HOP = 14000, 158
RATES = [48000, 44100]
LENGTHS = (30011, 9001, 1400)           # several frames and tiles; a chunk above max_chunk; J = 3 frames: all of it at close for K = 16
MAX_CHUNK = 4096
LEAD = 65                               # a trails what x gives by this much until the last push, as an input resampler's output
SIZES = {0: [1, 0, 7, 9001, 333], 1: [0, 9001], 2: [333, 1, 0, 7]}
MODES = [None, 0, 2, 16]                # gains= of the merger: 'keep', then 'follow' with K frames of smoothing
_cache = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mode_id(k):
    return "keep" if k is None else "K%d" % k


def _signals(rate):
    """Per rate, computed once and never modified: the three (x, a, b) on the GPU, the file path's result per mode, and on the host
    U(a), U(b) cut or zero-filled to n and the gains per K (what the float64 reference is fed)."""
    from sos_amd import audio_io
    if rate not in _cache:
        rng = np.random.default_rng(rate + 3)
        xs, As, bs = [], [], []
        for n in LENGTHS:
            x = rng.uniform(-1, 1, n).astype(np.float32)
            if n > 20000:
                x[11000:14000] = 0.0
            x = torch.from_numpy(x).cuda()
            a = audio_io.resample_device(x, rate, SR).clone()
            m = a.numel()
            env = torch.clamp(0.75 + 0.9 * torch.sin(torch.arange(m, device="cuda") / 400.0), min=0.0)      # 0 .. 1.65
            xs.append(x), As.append(a), bs.append((a * env)[:HOP * (m // HOP)].clone())
        frames = As[0][:HOP * (As[0].numel() // HOP)].view(-1, HOP)
        assert bool((frames == 0).all(dim=1).any()), "the setup needs a whole frame of a that is exactly zero (E_a == 0)"
        want, gains = {}, {}
        for K in MODES:
            g = None if K is None else audio_io.band_gains_batch_device(As, bs, HOP, K)
            want[K] = [y.clone() for y in audio_io.resample_merge_batch_device(xs, As, bs, SR, rate, g)]
            gains[K] = None if K is None else [s.cpu().numpy() for s in g]
        r0 = gains[0][0]                                            # K = 0: s is r
        assert r0.min() == 0.0 and r0.max() == 1.0 and ((r0 > 0.05) & (r0 < 0.95)).any(), "r reaches 0, the clip at 1 and the inside"
        fit = lambda t, n: np.concatenate([t.cpu().numpy()[:n], np.zeros(max(n - t.numel(), 0), dtype=np.float32)])      # noqa: E731
        ra = [fit(t, n) for t, n in zip(audio_io.resample_batch_device(As, SR, rate), LENGTHS)]
        rb = [fit(t, n) for t, n in zip(audio_io.resample_batch_device(bs, SR, rate, fix=False), LENGTHS)]
        _cache[rate] = dict(xs=xs, As=As, bs=bs, want=want, gains=gains, ra=ra, rb=rb)
    return _cache[rate]


def _steps(rate, n, m, mp, sizes, lag):
    """(steps (c_x, c_a, c_b), the largest ceil(n_x SR / rate) - m_b after a step): x in chunks of `sizes`, then the rest; a LEAD
    behind x; b behind a as `lag` says; a last step without x brings the rest of a and b."""
    n_x = m_a = m_b = worst = 0
    steps = []
    for c in list(sizes) + [n, None]:
        if c is None:
            new_a, new_b = m, mp
        else:
            c = min(c, n - n_x)
            n_x += c
            new_a = max(-(-n_x * SR // rate) - LEAD, 0)
            new_b = {"behind": min(new_a, mp), "bursts": min(10 * HOP * (new_a // (10 * HOP)), mp), "last": 0}[lag]
        steps.append((c or 0, new_a - m_a, new_b - m_b))
        m_a, m_b = new_a, new_b
        worst = max(worst, -(-n_x * SR // rate) - m_b)
    return steps, worst


def _plan(rate, lag, which=(0, 1, 2)):
    sig = _signals(rate)
    plans = {i: _steps(rate, LENGTHS[i], sig["As"][i].numel(), sig["bs"][i].numel(), SIZES[i], lag) for i in which}
    return {i: p[0] for i, p in plans.items()}, max(p[1] for p in plans.values())


def _feed(merger, sig, steps, slot_of, host=False):
    """Pushes signal i into slot slot_of[i] step by step, all slots in one call per step -> {i: the pushed pieces}."""
    at = {i: [0, 0, 0] for i in steps}
    outs = {i: [] for i in steps}
    for k in range(max(len(s) for s in steps.values())):
        chunks = {}
        for i, st in steps.items():
            if k < len(st):
                cut = [v[p:p + c] for v, p, c in zip((sig["xs"][i], sig["As"][i], sig["bs"][i]), at[i], st[k])]
                chunks[slot_of[i]] = tuple(c.cpu().numpy() for c in cut) if host and k % 2 else tuple(cut)
                at[i] = [p + c for p, c in zip(at[i], st[k])]
        got = merger.push(chunks)
        for i in steps:
            if slot_of[i] in got:
                y = got[slot_of[i]]
                assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 1
                outs[i].append(y)
    return outs


@pytest.mark.parametrize("lag", ["behind", "bursts", "last"])
@pytest.mark.parametrize("K", MODES, ids=_mode_id)
@pytest.mark.parametrize("rate", RATES)
def test_three_streams_in_chunks_are_the_file_path_bit_for_bit(rate, K, lag):
    from sos_amd import audio_io
    sig = _signals(rate)
    steps, worst = _plan(rate, lag)
    merger = audio_io.StreamBandMerger(3, SR, rate, worst, gains=K, hop=HOP, max_chunk=MAX_CHUNK)
    if lag == "behind" and K != 16:
        assert merger.capacity < 9001                              # the 9 001-sample chunk goes in pieces
    slot_of = {0: 2, 1: 0, 2: 1}
    outs = _feed(merger, sig, steps, slot_of, host=True)
    rest = merger.close([slot_of[i] for i in (1, 2, 0)])
    for i, n in enumerate(LENGTHS):
        got = torch.cat(outs[i] + [rest[slot_of[i]]])
        want = sig["want"][K][i]
        assert got.shape == want.shape == (n,)
        same = torch.equal(_bits(got), _bits(want))
        assert same, (rate, K, lag, i, int((_bits(got) != _bits(want)).nonzero()[0]))
        before_close = sum(y.numel() for y in outs[i])
        if lag == "behind" and i < 2 and K != 16:                   # most of a long stream comes out of push()
            assert before_close >= n - (rate / SR) * ((0 if K is None else K + 2) * HOP + LEAD + 66 + 2 * HOP) - 2
        if i == 2 and K == 16:
            assert before_close == 0                                # J = 3 < K: nothing is final before the end is known
        if K is not None:                                           # and within the rounding bound of the float64 reference
            x = sig["xs"][i].cpu().numpy().astype(np.float64)
            ra, rb = sig["ra"][i], sig["rb"][i]
            ref = B.merge(x, ra, rb, B.interp(sig["gains"][K][i], n, SR, rate, HOP))
            bound = 2.0 ** -22 * (np.abs(x - ra) + np.abs(rb.astype(np.float64)))
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            print(rate, _mode_id(K), lag, n, "max error / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound)
    assert merger.count == [None] * 3


def test_slots_are_independent_can_be_used_again_and_dropped():
    from sos_amd import audio_io
    rate, K = 44100, 2
    sig = _signals(rate)
    steps, worst = _plan(rate, "bursts")
    alone = audio_io.StreamBandMerger(4, SR, rate, worst, gains=K, hop=HOP, max_chunk=MAX_CHUNK)
    one = _feed(alone, sig, {1: steps[1]}, {1: 3})[1]
    among = audio_io.StreamBandMerger(4, SR, rate, worst, gains=K, hop=HOP, max_chunk=MAX_CHUNK)
    three = _feed(among, sig, steps, {0: 0, 1: 3, 2: 1})
    assert len(one) == len(three[1]) and sum(y.numel() for y in one) > 0
    for p, q in zip(one, three[1]):                                  # the same pieces alone and among others
        assert torch.equal(_bits(p), _bits(q))
    want = sig["want"][K]
    assert torch.equal(_bits(torch.cat(one + [alone.close(3)[3]])), _bits(want[1]))
    rest = among.close([3, 1])
    assert torch.equal(_bits(torch.cat(three[1] + [rest[3]])), _bits(want[1]))
    assert torch.equal(_bits(torch.cat(three[2] + [rest[1]])), _bits(want[2]))
    # slot 3's rings still hold stream 1: a new stream there starts at 0 and does not see it; slot 0 is still open beside it
    again = _feed(among, sig, {2: steps[2]}, {2: 3})[2]
    assert torch.equal(_bits(torch.cat(again + [among.close(3)[3]])), _bits(want[2]))
    assert torch.equal(_bits(torch.cat(three[0] + [among.close(0)[0]])), _bits(want[0]))
    among.push({2: (sig["xs"][1][:900], sig["As"][1][:100], sig["bs"][1][:50])})
    among.drop([2])
    assert among.count == [None] * 4
    with pytest.raises(ValueError, match="slot 2 has no open stream"):
        among.drop(2)
    again = _feed(among, sig, {1: steps[1]}, {1: 2})[1]
    assert torch.equal(_bits(torch.cat(again + [among.close(2)[2]])), _bits(want[1]))


def _sync_warnings(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in rec)


def test_nothing_waits_for_the_device_after_a_warm_up_session():
    from sos_amd import audio_io
    rate, K = 48000, 2
    sig = _signals(rate)
    steps, worst = _plan(rate, "behind", which=(1, 2))

    def session():
        merger = audio_io.StreamBandMerger(2, SR, rate, worst, gains=K, hop=HOP, max_chunk=MAX_CHUNK)
        outs = _feed(merger, sig, steps, {1: 0, 2: 1})
        rest = merger.close([0, 1])
        return [torch.cat(outs[i] + [rest[s]]) for i, s in ((1, 0), (2, 1))]

    session()                                                   # filter table, code objects, pinned staging
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = session()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for y, i in zip(outs, (1, 2)):
        assert torch.equal(_bits(y), _bits(sig["want"][K][i]))
    x, a = sig["xs"][0], sig["As"][0]
    few, many = (audio_io.StreamBandMerger(s, SR, rate, 2000, gains=K, hop=HOP) for s in (2, 64))
    chunk = (x[:4800], a[:1335], a[:1200])
    w2 = _sync_warnings(lambda: few.push({s: chunk for s in range(2)}))
    w64 = _sync_warnings(lambda: many.push({s: chunk for s in range(64)}))
    print(f"synchronisation warnings of one push: 2 slots: {w2}, 64 slots: {w64}")
    assert w2 == w64 == 0


def test_refusals_come_before_any_launch():
    from sos_amd import _lib, audio_io
    rate = 48000
    sig = _signals(rate)
    x, a, b = sig["xs"][1], sig["As"][1], sig["bs"][1]
    merger = audio_io.StreamBandMerger(3, SR, rate, 500, gains=2, hop=HOP, max_chunk=MAX_CHUNK)
    head = merger.push({0: (x[:2000], a[:500], b[:480]), 1: (x[:10], a[:0], b[:0])})[0]
    assert head.numel() > 0
    kept, done = head.clone(), list(merger.t_done)
    h = _lib.lib()
    d_good = torch.zeros((1, 10), dtype=torch.int64, device="cuda")      # the device table is never the corrupted one (and never read)
    out = torch.empty(64, dtype=torch.float32, device="cuda")
    cap, rcap = merger.capacity, merger.frames
    x_f64 = x.cpu().numpy().astype(np.float64)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(ValueError, match="must exceed low_sr"):
            audio_io.StreamBandMerger(1, SR, SR, 100)
        with pytest.raises(ValueError, match="must exceed low_sr"):
            audio_io.StreamBandMerger(1, SR, 8000, 100)
        with pytest.raises(ValueError, match="res_type 'kaiser_fast' is not supported"):
            audio_io.StreamBandMerger(1, SR, rate, 100, res_type="kaiser_fast")
        for bad in (-1, 17, 2.0, True):
            with pytest.raises(ValueError, match="within 0 .. 16"):
                audio_io.StreamBandMerger(1, SR, rate, 100, gains=bad)
        for slots in (0, 21846):
            with pytest.raises(ValueError, match="slots"):
                audio_io.StreamBandMerger(slots, SR, rate, 100)
        for kw in (dict(max_lag=-1), dict(max_lag=1, max_chunk=0), dict(max_lag=1, hop=0)):
            with pytest.raises(ValueError, match="max_lag is at least 0"):
                audio_io.StreamBandMerger(1, SR, rate, **kw)
        for slot in (3, -1, "0"):
            with pytest.raises(ValueError, match="unknown slot"):
                merger.push({slot: (x[:1], a[:0], b[:0])})
        for chunk in (x[None], x.double(), x_f64, [0.0] * 10):
            with pytest.raises(ValueError, match="1-D float32"):
                merger.push({2: (chunk, a[:0], b[:0])})
            with pytest.raises(ValueError, match="1-D float32"):
                merger.push({2: (x[:100], a[:0], chunk)})
        with pytest.raises(ValueError, match="three chunks"):
            merger.push({2: x[:100]})
        with pytest.raises(ValueError, match="slot 0: .*b may not run ahead of a"):
            merger.push({2: (x[:100], a[:20], b[:10]), 0: (x[2000:2100], a[500:510], b[480:511])})
        with pytest.raises(ValueError, match="slot 2: .*a not ahead of what x gives"):
            merger.push({2: (x[:100], a[:31], b[:0])})              # 100 samples at 48 kHz give 30
        with pytest.raises(ValueError, match="slot 0: .*at most max_lag = 500"):
            merger.push({0: (x[2000:4000], a[500:510], b[480:490])})
        assert merger.count == [(2000, 500, 480), (10, 0, 0), None] and merger.t_done == done        # nothing was opened or moved
        for call in (merger.close, merger.drop):
            with pytest.raises(ValueError, match="slot 2 has no open stream"):
                call([0, 2])
            with pytest.raises(ValueError, match="named twice"):
                call([0, 0])
        merger.push({2: (x[:300], a[:88], b[:88])})                  # a stream that could be closed
        with pytest.raises(ValueError, match="slot 1: 10 samples at 48000 Hz are not covered by the 0 at 14000 Hz"):
            merger.close([2, 1])                                    # slot 1 is named and free again, slot 2 stays open
        assert merger.count == [(2000, 500, 480), None, (300, 88, 88)]
        merger.drop(2)
        # the ABI refuses a bad HOST row with SOS_EINVAL and names it
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
                           ([[0, 0, 10, 2000, 500, 400, 10, -1, 1, 0]], "row 0 reads frames of r its ring of frames does not hold"),
                           ([[0, 0, 10, 2000, 500, 400, 10, 3, 4, 0]], "row 0 reads frames of r its ring of frames does not hold"),
                           ([[0, 0, 10, 2000, 500, 400, 10, -1, rcap + 1, 0]], "row 0 reads frames of r its ring of frames does not hold"),
                           ([ok, [1, 0, 10, 2000, 500, 400, 10, -1, 3, 10], [0, 10, 20, 2000, 500, 400, 20, -1, 3, 20]],
                            "row 2 names slot 0, which an earlier row")):
            tab = np.asarray(rows, dtype=np.int64)
            rc = h.sos_stream_band_merge_f32(_lib.ptr(merger.ring), 3, cap, _lib.ptr(merger.rring), rcap, _lib.ptr(d_good),
                                             tab.ctypes.data, len(rows), merger.ratio, _lib.ptr(merger.win), merger.win.numel(),
                                             merger.num_table, HOP, 2, _lib.ptr(out), out.numel(), None)
            assert rc == -22 and told in h.sos_last_error().decode(), (rows, rc, h.sos_last_error())
        # ratio rows {slot, j_lo, j_hi, m_a, m_b}
        for rows, told in (([[3, 0, 1, 500, 400]], "row 0 names a slot outside the slots"),
                           ([[0, 2, 1, 500, 400]], "row 0 has a range that is none"),
                           ([[0, 0, 5, 500, 400]], "row 0 has a range that is none, or frames"),
                           ([[0, 0, 1, 400, 500]], "row 0 has counts that do not fit"),
                           ([[0, 0, 1, cap + 1, 400]], "row 0 reads samples of a or b their rings do not hold"),
                           ([[0, 0, 1, 500, 400], [0, 1, 2, 500, 400]], "row 1 names slot 0, which an earlier row")):
            tab = np.asarray(rows, dtype=np.int64)
            rc = h.sos_stream_band_ratio_f64(_lib.ptr(merger.ring), 3, cap, _lib.ptr(d_good), tab.ctypes.data, len(rows), HOP,
                                             _lib.ptr(merger.rring), rcap, None)
            assert rc == -22 and told in h.sos_last_error().decode(), (rows, rc, h.sos_last_error())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(_bits(head), _bits(kept))                    # what was returned is untouched
    # slot 0 streams on as ever, and the freed slot serves a new stream
    n, m, mp = x.numel(), a.numel(), b.numel()
    tail = [merger.push({0: (x[2000:], a[500:m - 70], b[480:m - 400])})[0], merger.push({0: (x[:0], a[m - 70:], b[m - 400:])})[0]]
    assert torch.equal(_bits(torch.cat([head] + tail + [merger.close(0)[0]])), _bits(sig["want"][2][1]))
    got = torch.cat([merger.push({1: (sig["xs"][2], sig["As"][2], sig["bs"][2])})[1], merger.close(1)[1]])
    assert torch.equal(_bits(got), _bits(sig["want"][2][2]))
