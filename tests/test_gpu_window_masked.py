"""sos_window_stage_masked_f32 (csrc/ragged_window.hip): windows of recordings staged together with their noise intervals, the
mask rule evaluated in the RECORDING's coordinates.  The reference is tools.ragged_stage on the whole recordings: the rows must
be slices of its full-length `wave` and `masked`, bit for bit, zero beyond the window's samples.  Kernel level, tiny recordings:
the kernel knows nothing of the hop or of MIN_FRAMES."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
SPARE = 16
RATIOS = [14000 / 30.0, 560.0, 7.3]                # 7.3: the ratio < 16 branch of mask_sample


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _clip_table(ns, nb):
    tab = np.zeros((len(ns), 4), np.int64)
    tab[:, 1], tab[:, 3] = ns, nb
    tab[1:, 0], tab[1:, 2] = np.cumsum(ns)[:-1], np.cumsum(nb)[:-1]
    return tab


def _recordings(ns, ratios, seed):
    """Recordings of `ns` samples with random decisions, int(n / ratio) + 1 frames each (the last frame reaches past the end):
    (flat, bits, clip table) on the host, and tools.ragged_stage's full-length wave / masked rows."""
    from sos_amd import tools
    rng = np.random.default_rng(seed)
    nb = [int(n / r) + 1 for n, r in zip(ns, ratios)]
    flat = rng.standard_normal(sum(ns)).astype(np.float32)
    bits = rng.integers(0, 2, sum(nb)).astype(np.uint8)
    clips = _clip_table(ns, nb)
    wave, masked, mask = tools.ragged_stage(torch.from_numpy(flat).cuda(), clips, max(ns), torch.from_numpy(bits).cuda(), ratios)
    return flat, bits, clips, wave.cpu().numpy(), masked.cpu().numpy(), mask.cpu().numpy()


def _windows(clips, spans):
    """Window rows {recording, source offset, samples, -, -, -, window start, row, -1, -1} for (recording, start, samples)."""
    tab = np.zeros((len(spans), 10), np.int64)
    for w, (r, start, n) in enumerate(spans):
        tab[w] = (r, clips[r, 0] + start, n, 0, 0, 0, start, w, -1, -1)
    return tab


def _spans(n, ratio):
    """Windows of a recording of n samples: starts on every residue mod 4, one that ends at the last sample, one that spans a
    frame edge, one of a single sample, one of the whole recording."""
    edge = int(ratio * max(1, int(n / ratio) // 2))                          # a frame edge inside the recording
    spans = [(0, n), (1, min(n - 1, 1001)), (2, min(n - 2, 333)), (3, min(n - 3, 64)), (n - min(n, 203), min(n, 203)),
             (max(edge - 9, 0), 21), (n - 1, 1), (5, 6)]
    assert all(0 <= s and s + m <= n for s, m in spans)
    return spans


@pytest.mark.parametrize("stride_extra", [0, 3], ids=["stride%4=0", "stride%4=3"])
@pytest.mark.parametrize("ratio", RATIOS, ids=["466.67", "560", "7.3"])
def test_rows_are_slices_of_the_full_length_stage(ratio, stride_extra):
    from sos_amd import tools
    n = 2803 if ratio > 16 else 411
    flat, bits, clips, wave, masked, mask = _recordings([n], [ratio], seed=int(ratio))
    assert 0 < mask.sum() < n
    spans = _spans(n, ratio)
    tab = _windows(clips, [(0, s, m) for s, m in spans])
    stride = -(-n // 4) * 4 + stride_extra
    assert stride % 4 == stride_extra and {s % 4 for s, _ in spans} == {0, 1, 2, 3}
    w, m = tools.window_stage_masked(torch.from_numpy(flat).cuda(), torch.from_numpy(bits).cuda(), clips, [ratio], tab, stride)
    w, m = w.cpu().numpy(), m.cpu().numpy()
    assert w.shape == m.shape == (len(spans), stride)
    for k, (s, cnt) in enumerate(spans):
        assert _same_bits(w[k, :cnt], wave[0, s:s + cnt]) and _same_bits(m[k, :cnt], masked[0, s:s + cnt]), (k, s, cnt)
        assert _same_bits(m[k, :cnt], flat[s:s + cnt] * mask[s:s + cnt])
        assert not w[k, cnt:].any() and not m[k, cnt:].any(), k
    # the run-flip at the recording's end is the recording's, not the window's: the window that ends at the last sample and the
    # windows that end before it agree with the full-length mask wherever they overlap (checked above); and the mask does flip
    # somewhere (with 57 random frames of 7.3 samples a run shorter than five samples exists)
    if ratio < 16:
        assert (_premask(bits, ratio, n) != mask).any()


def _premask(bits, ratio, n):
    """The mask before the short-run flip (mask_rule.h: premask), float64 like Python's."""
    pre = np.zeros(n, np.float32)
    for i, b in enumerate(bits):
        lo, hi = int(i * ratio), int((i + 1) * ratio - 1)
        if b == 0:
            pre[lo:min(hi, n)] = 1
    return pre


def test_two_recordings_with_different_ratios_in_one_launch():
    from sos_amd import tools
    ns, ratios = [2803, 1501, 411], [14000 / 30.0, 560.0, 7.3]
    flat, bits, clips, wave, masked, mask = _recordings(ns, ratios, seed=4)
    assert clips[1, 0] % 4 and clips[2, 0] % 4 == 0                           # recordings on both alignments
    spans = [(r, s, m) for r, (n, q) in enumerate(zip(ns, ratios)) for s, m in _spans(n, q)]
    order = np.random.default_rng(5).permutation(len(spans))
    spans = [spans[i] for i in order]                                          # windows of the recordings interleaved
    tab = _windows(clips, spans)
    d_flat, d_bits = torch.from_numpy(flat).cuda(), torch.from_numpy(bits).cuda()
    w, m = tools.window_stage_masked(d_flat, d_bits, clips, ratios, tab, 2804)
    w, m = w.cpu().numpy(), m.cpu().numpy()
    for k, (r, s, cnt) in enumerate(spans):
        assert _same_bits(w[k, :cnt], wave[r, s:s + cnt]) and _same_bits(m[k, :cnt], masked[r, s:s + cnt]), (k, r, s, cnt)
        assert not w[k, cnt:].any() and not m[k, cnt:].any(), k
    # a window alone gives the same bits as in the batch
    for k in (0, 7, len(spans) - 1):
        w1, m1 = tools.window_stage_masked(d_flat, d_bits, clips, ratios, tab[k:k + 1], 2807)
        assert _same_bits(w1.cpu().numpy()[0, :2804], w[k]) and _same_bits(m1.cpu().numpy()[0, :2804], m[k])


def _raw(*args):
    from sos_amd import _lib as L
    rc = L.lib().sos_window_stage_masked_f32(*args, L.stream_ptr())
    return rc, L.lib().sos_last_error().decode()


def _small():
    ns, ratios = [1501, 411], [560.0, 7.3]
    flat, bits, clips, wave, masked, mask = _recordings(ns, ratios, seed=6)
    tab = _windows(clips, [(0, 0, 700), (0, 613, 888), (1, 3, 400), (1, 200, 211)])
    return ns, np.asarray(ratios), flat, bits, clips, tab


def test_host_refusals_name_the_window_or_the_recording():
    from sos_amd import _lib as L
    ns, rat, flat, bits, clips, tab = _small()
    W, stride = len(tab), 888
    d_flat, d_bits = torch.from_numpy(flat).cuda(), torch.from_numpy(bits).cuda()
    d_clips, d_rat, d_tab = (torch.from_numpy(a).cuda() for a in (clips, rat, tab))
    wave, masked = torch.zeros((W, stride), device="cuda"), torch.zeros((W, stride), device="cuda")

    def call(t=tab, c=clips, q=rat, x=d_flat, b=d_bits, nrec=2, nwin=W, stride=stride, wave=wave, masked=masked, dev=d_tab):
        t, c, q = (np.ascontiguousarray(a) for a in (t, c, q))
        return _raw(L.ptr(x), L.ptr(b), L.ptr(d_clips), c.ctypes.data, L.ptr(d_rat), q.ctypes.data, nrec, L.ptr(dev), t.ctypes.data,
                    nwin, stride, L.ptr(wave), L.ptr(masked))

    def changed(a, i, col, value):
        a = a.copy()
        if a.ndim == 1:
            a[i] = value
        else:
            a[i, col] = value
        return a

    assert call()[0] == 0
    for kw in (dict(x=None), dict(b=None), dict(wave=None), dict(masked=None), dict(dev=None)):
        rc, msg = call(**kw)
        assert rc == -22 and "null pointer" in msg, msg
    for kw in (dict(nwin=0), dict(nwin=65536), dict(stride=0), dict(nrec=0), dict(nrec=65536)):
        rc, msg = call(**kw)
        assert rc == -22 and "bad args" in msg, (kw, msg)
    for what, kw, name in (("more samples than the stride", dict(stride=887), "window 1 "),
                           ("a recording that does not exist", dict(t=changed(tab, 2, 0, 2)), "window 2 "),
                           ("a negative recording", dict(t=changed(tab, 0, 0, -1)), "window 0 "),
                           ("a window past its recording's end", dict(t=changed(tab, 1, 2, 889), stride=889), "window 1 "),
                           ("a negative start", dict(t=changed(changed(tab, 2, 6, -1), 2, 1, tab[2, 1] - 4)), "window 2 "),
                           ("a source offset that is not the start", dict(t=changed(tab, 3, 1, tab[3, 1] + 1)), "window 3 "),
                           ("negative samples", dict(t=changed(tab, 0, 2, -1)), "window 0 "),
                           ("a recording outside the samples", dict(c=changed(clips, 1, 0, clips[1, 0] + 1)), "recording 1 "),
                           ("a recording outside the frames", dict(c=changed(clips, 0, 2, clips[1, 3] + 1)), "recording 0 "),
                           ("negative samples of a recording", dict(c=changed(clips, 0, 1, -1)), "recording 0 "),
                           ("a ratio of one", dict(q=changed(rat, 1, 0, 1.0)), "recording 1 "),
                           ("a ratio that is no number", dict(q=changed(rat, 0, 0, np.nan)), "recording 0 ")):
        rc, msg = call(**kw)
        assert rc == -22 and msg.startswith("sos_window_stage_masked_f32: ") and name in msg, (what, msg)


def _spared(a, fill=0):
    a = np.asarray(a).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(SPARE, fill, a.dtype)])).cuda()


def test_kernel_skips_a_device_entry_that_leaves_the_hosts_sizes():
    """The device rule: the host tables are correct, a DEVICE table differs in one entry.  The call succeeds, the rows of the
    windows that need the entry are left as they were, every other row is what the unaltered call gives, nothing past the
    buffers is written (spare elements behind every buffer keep a wrongly followed entry inside allocated memory)."""
    from sos_amd import _lib as L
    ns, rat, flat, bits, clips, tab = _small()
    W, stride = len(tab), 888
    d_flat, d_bits = _spared(flat), _spared(bits)

    def run(t=tab, c=clips, q=rat):
        wave = torch.full((W * stride + SPARE,), SENTINEL, device="cuda")
        masked = torch.full((W * stride + SPARE,), SENTINEL, device="cuda")
        d = [_spared(a) for a in (t, c, q)]
        rc = L.lib().sos_window_stage_masked_f32(L.ptr(d_flat), L.ptr(d_bits), L.ptr(d[1]), clips.ctypes.data, L.ptr(d[2]),
                                                 rat.ctypes.data, 2, L.ptr(d[0]), tab.ctypes.data, W, stride, L.ptr(wave),
                                                 L.ptr(masked), L.stream_ptr())
        assert rc == 0
        return wave.cpu().numpy(), masked.cpu().numpy()

    def changed(a, i, col, value):
        a = a.copy()
        if a.ndim == 1:
            a[i] = value
        else:
            a[i, col] = value
        return a

    base = run()
    assert all(not (b[:W * stride] == SENTINEL).any() and (b[W * stride:] == SENTINEL).all() for b in base)

    def check(got, skipped):
        for g, b in zip(got, base):
            assert (g[W * stride:] == SENTINEL).all()
            for w in range(W):
                row = g[w * stride:(w + 1) * stride]
                assert (row == SENTINEL).all() if w in skipped else _same_bits(row, b[w * stride:(w + 1) * stride]), (w, skipped)

    for w, col, value in ((1, 2, stride + 1), (2, 0, 2), (2, 0, -1), (3, 6, 201), (0, 1, 1), (3, 2, -1), (1, 6, -1)):
        check(run(t=changed(tab, w, col, value)), {w})
    # a recording's entry: every window of that recording
    for r, col, value in ((1, 0, clips[1, 0] + 1), (0, 1, -1), (1, 2, clips[1, 2] + 1), (0, 3, len(bits) + 1)):
        check(run(c=changed(clips, r, col, value)), {0, 1} if r == 0 else {2, 3})
    check(run(q=changed(rat, 0, 0, 1.0)), {0, 1})
    check(run(q=changed(rat, 1, 0, np.nan)), {2, 3})
