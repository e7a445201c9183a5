"""sos_ragged_stage_f32 / sos_ragged_unpack_f32 (csrc/ragged_io.hip): a ragged group of clips staged for the networks in one
launch, and padded result rows gathered into one back-to-back buffer.  The reference of the mask is tools.bits_to_mask_batch
called once per clip at that clip's ratio (the same rule through csrc/mask_rule.h): every comparison is bit for bit.  The
integer rule itself is checked against oracle.frontend.convert_bitstreammask_to_audiomask in both ratio regimes."""
import numpy as np
import pytest
import torch

from oracle import frontend as ofe

pytestmark = pytest.mark.gpu

LENGTHS = (1, 255, 256, 257, 4097, 11200)
SENTINEL = -77.0


def _group():
    """Six clips: every length of LENGTHS, the four ratios (7.5 takes the general path below 16), and the frame patterns:
    frames running past the samples (clips 0, 4), ending before them (3), all silent (4), all speech (2), alternating every
    frame at 7.5 samples per frame (1), random (3, 5).  The rule leaves the last sample of every frame out of its interval, so
    two silent frames in a row are separated by a run of one or two samples: the runs the short-run flip turns over (3, 4)."""
    rng = np.random.default_rng(21)
    ratios = [14000 / 30, 7.5, 14000 / 25, 7.5, 16000 / 29.97, 14000 / 30]
    bits = [np.zeros(1, np.uint8),
            (np.arange(34) % 2).astype(np.uint8),
            np.ones(1, np.uint8),
            rng.integers(0, 2, 20).astype(np.uint8),
            np.zeros(8, np.uint8),
            rng.integers(0, 2, 24).astype(np.uint8)]
    clips = [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]
    assert 20 * 7.5 < 257 and 8 * 16000 / 29.97 > 4097 and 14000 / 30 > 1
    return clips, bits, ratios


@pytest.fixture(scope="module")
def reference():
    """Per clip: (mask, masked) of tools.bits_to_mask_batch for that clip alone, as host arrays.  Computed once."""
    from sos_amd import tools
    clips, bits, ratios = _group()
    ref = []
    for c, b, r in zip(clips, bits, ratios):
        m, mk = tools.bits_to_mask_batch(torch.from_numpy(b[None]).cuda(), r, len(c), torch.from_numpy(c[None]).cuda())
        ref.append((m[0].cpu().numpy(), mk[0].cpu().numpy()))
    return clips, bits, ratios, ref


def _table(ns, nb):
    ends, bends = np.cumsum(ns), np.cumsum(nb)
    return np.stack([ends - ns, ns, bends - nb, nb], axis=1).astype(np.int64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _stage(clips, bits, ratios, stride):
    from sos_amd import tools
    ns, nb = [len(c) for c in clips], [len(b) for b in bits]
    wave, masked, mask = tools.ragged_stage(torch.from_numpy(np.concatenate(clips)).cuda(), _table(ns, nb), stride,
                                            torch.from_numpy(np.concatenate(bits)).cuda(), ratios)
    return wave.cpu().numpy(), masked.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("stride", [11200, 11203], ids=["stride%4=0", "stride%4=3"])
def test_stage_equals_bits_to_mask_per_clip(reference, stride, order):
    clips, bits, ratios, ref = reference
    idx = list(range(len(clips)))[::-1] if order == "reversed" else list(range(len(clips)))
    wave, masked, mask = _stage([clips[i] for i in idx], [bits[i] for i in idx], [ratios[i] for i in idx], stride)
    assert wave.shape == masked.shape == (len(clips), stride)
    pos = 0
    offsets = []
    for row, i in enumerate(idx):
        n = len(clips[i])
        offsets.append(pos)
        assert _same_bits(mask[pos:pos + n], ref[i][0]), (i, "mask")
        assert _same_bits(masked[row, :n], ref[i][1]), (i, "masked")
        assert _same_bits(wave[row, :n], clips[i]), (i, "wave")
        assert not wave[row, n:].any() and not masked[row, n:].any(), (i, "zero fill")
        pos += n
    assert pos == mask.size
    assert any(o % 4 for o in offsets) and any(o % 4 == 0 and o for o in offsets)        # both access paths were taken
    assert 0 < sum(float(m.sum()) for m, _ in ref) < pos                                 # both mask values occur


def test_pack_only_writes_the_wave_and_nothing_else(reference):
    from sos_amd import _lib as L
    from sos_amd import tools
    clips, bits, _, _ = reference
    ns = [len(c) for c in clips]
    flat = torch.from_numpy(np.concatenate(clips)).cuda()
    wave = tools.ragged_stage(flat, _table(ns, [0] * len(ns)), 11200)
    assert torch.is_tensor(wave) and wave.shape == (len(ns), 11200)
    host = wave.cpu().numpy()
    for row, c in enumerate(clips):
        assert _same_bits(host[row, :len(c)], c) and not host[row, len(c):].any()
    # the same call on the C ABI with buffers for masked and mask passed anyway: without frame decisions they stay as they were
    tab = _table(ns, [len(b) for b in bits])
    d_tab = torch.from_numpy(tab).cuda()
    out = torch.full((len(ns), 11200), SENTINEL, device="cuda")
    masked, mask = torch.full_like(out, SENTINEL), torch.full_like(flat, SENTINEL)
    L.check(L.lib().sos_ragged_stage_f32(L.ptr(flat), L.ptr(d_tab), tab.ctypes.data, len(ns), None, None, None, 11200,
                                         L.ptr(out), L.ptr(masked), L.ptr(mask), L.stream_ptr()))
    assert torch.equal(out, wave)
    assert bool((masked == SENTINEL).all()) and bool((mask == SENTINEL).all())


def test_unpack_inverts_stage_and_gathers_rows_in_any_order(reference):
    from sos_amd import tools
    clips, _, _, _ = reference
    ns = [len(c) for c in clips]
    flat = torch.from_numpy(np.concatenate(clips)).cuda()
    for stride in (11200, 11203):
        wave = tools.ragged_stage(flat, _table(ns, [0] * len(ns)), stride)
        ends = np.cumsum(ns)
        back = tools.ragged_unpack(wave, np.stack([np.arange(len(ns)), ns, ends - ns], axis=1))
        assert torch.equal(back, flat)
        # rows in another order, one twice, valid < stride, output offsets 1001, 1256, 1263 (not multiples of four)
        picks = [(5, 1001), (3, 255), (5, 7), (0, 1), (4, 4096)]
        offs = np.cumsum([0] + [n for _, n in picks[:-1]])
        got = tools.ragged_unpack(wave, [(r, n, o) for (r, n), o in zip(picks, offs)]).cpu().numpy()
        want = np.concatenate([clips[r][:n] for r, n in picks])
        assert _same_bits(got, want)


def test_a_clip_past_the_buffer_is_refused_on_the_host(reference):
    from sos_amd import tools
    clips, bits, ratios, _ = reference
    ns, nb = [len(c) for c in clips], [len(b) for b in bits]
    flat = torch.from_numpy(np.concatenate(clips)).cuda()
    d_bits = torch.from_numpy(np.concatenate(bits)).cuda()
    tab = _table(ns, nb)
    tab[-1, 0] += 1                                   # the last clip ends one sample past the samples the table sums to
    with pytest.raises(RuntimeError, match=r"rc=-22.*clip 5"):
        tools.ragged_stage(flat, tab, 11200, d_bits, ratios)
    tab = _table(ns, nb)
    tab[-1, 2] += 1                                   # ... and one frame past the frame decisions
    with pytest.raises(RuntimeError, match=r"rc=-22.*clip 5"):
        tools.ragged_stage(flat, tab, 11200, d_bits, ratios)
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        tools.ragged_stage(flat, _table(ns, nb), 11199, d_bits, ratios)          # a clip longer than the stride
    wave = tools.ragged_stage(flat, _table(ns, [0] * len(ns)), 11200)
    with pytest.raises(RuntimeError, match=r"rc=-22.*entry 1"):
        tools.ragged_unpack(wave, [(0, 1, 0), (5, 11200, 2)])                    # output 2 + 11200 > 11201
    with pytest.raises(RuntimeError, match=r"rc=-22.*entry 0"):
        tools.ragged_unpack(wave, [(6, 1, 0)])                                   # row 6 of 6


@pytest.mark.parametrize("ratio", [14000 / 30, 7.5], ids=["ratio>=16", "ratio<16"])
def test_bits_to_mask_still_is_the_integer_rule(ratio):
    """After the move of the arithmetic into mask_rule.h: sos_bits_to_mask against the oracle's integer rule, bit-exactly."""
    from sos_amd import tools
    rng = np.random.default_rng(4)
    nfr = 40
    n = int(nfr * ratio) + 9                          # samples past the last frame too
    for bits in (rng.integers(0, 2, nfr), np.arange(nfr) % 2, np.zeros(nfr, np.int64)):
        want = ofe.convert_bitstreammask_to_audiomask(np.zeros(n, np.float32), ratio, [int(b) for b in bits])
        got = tools.bits_to_mask_batch(torch.from_numpy(bits.astype(np.uint8)[None]).cuda(), ratio, n)[0].cpu().numpy()
        assert np.array_equal(got, want)


SPARE = 16                                                # elements past what the table sums to, in every buffer


def _spared(a, fill=0):
    """`a` on the GPU with SPARE further elements behind it: an entry that is wrongly followed one element past the totals still
    touches allocated memory only, and shows up as a wrong value."""
    a = np.asarray(a).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(SPARE, fill, a.dtype)])).cuda()


def test_stage_kernel_skips_a_device_entry_outside_the_totals(reference):
    """The device rule of ragged_stage_kernel: the host table is correct, the DEVICE table differs in one entry of clip 1.  The
    call succeeds, clip 1's rows and mask span are left as they were, every other clip is what the unaltered call gives."""
    from sos_amd import _lib as L
    clips, bits, ratios, _ = reference
    ns, nb = [len(c) for c in clips], [len(b) for b in bits]
    B, stride, total, total_bits = len(ns), 11200, sum(ns), sum(nb)
    tab, rat = _table(ns, nb), np.asarray(ratios, dtype=np.float64)
    flat, d_bits, d_rat = _spared(np.concatenate(clips)), _spared(np.concatenate(bits)), torch.from_numpy(rat).cuda()

    def run(d_tab):
        wave = torch.full((B * stride + SPARE,), SENTINEL, device="cuda")
        masked, mask = torch.full_like(wave, SENTINEL), torch.full((total + SPARE,), SENTINEL, device="cuda")
        rc = L.lib().sos_ragged_stage_f32(L.ptr(flat), L.ptr(d_tab), tab.ctypes.data, B, L.ptr(d_bits), L.ptr(d_rat), rat.ctypes.data,
                                          stride, L.ptr(wave), L.ptr(masked), L.ptr(mask), L.stream_ptr())
        return rc, wave.cpu().numpy(), masked.cpu().numpy(), mask.cpu().numpy()

    rc, *base = run(torch.from_numpy(tab).cuda())
    assert rc == 0 and not any((a[:-SPARE] == SENTINEL).all() for a in base)
    o1, n1 = int(tab[1, 0]), ns[1]
    for what, col, value in (("sample offset", 0, total - n1 + 1), ("samples", 1, stride + 1), ("frame offset", 2, total_bits - nb[1] + 1)):
        d_tab = torch.from_numpy(tab).cuda()
        d_tab[1, col] = value
        rc, *got = run(d_tab)
        assert rc == 0, what
        for g, b, name in zip(got, base, ("wave", "masked", "mask")):
            lo, hi = (o1, o1 + n1) if name == "mask" else (stride, 2 * stride)          # clip 1's span / row
            assert (g[lo:hi] == SENTINEL).all(), (what, name)
            assert _same_bits(g[:lo], b[:lo]) and _same_bits(g[hi:], b[hi:]), (what, name)
            assert (g[-SPARE:] == SENTINEL).all(), (what, name)


def test_unpack_kernel_skips_a_device_entry_outside_the_totals(reference):
    """The same for ragged_unpack_kernel: a row that does not exist, an output span one sample past the total."""
    from sos_amd import _lib as L
    clips, _, _, _ = reference
    ns = [len(c) for c in clips]
    B, stride, total = len(ns), 11200, sum(ns)
    rows = np.zeros((B + 1, stride), np.float32)          # a spare row: "row = n_rows", wrongly followed, reads it
    for r, c in enumerate(clips):
        rows[r, :len(c)] = c
    d_rows = _spared(rows)
    offs = np.cumsum(ns) - ns
    tab = np.ascontiguousarray(np.stack([np.arange(B), ns, offs], axis=1).astype(np.int64))

    def run(d_tab):
        out = torch.full((total + SPARE,), SENTINEL, device="cuda")
        rc = L.lib().sos_ragged_unpack_f32(L.ptr(d_rows), B, stride, L.ptr(d_tab), tab.ctypes.data, B, L.ptr(out), L.stream_ptr())
        return rc, out.cpu().numpy()

    rc, base = run(torch.from_numpy(tab).cuda())
    assert rc == 0 and _same_bits(base[:total], np.concatenate(clips))
    lo, hi = int(offs[1]), int(offs[1]) + ns[1]
    for what, col, value in (("row", 0, B), ("output offset", 2, total - ns[1] + 1)):
        d_tab = torch.from_numpy(tab).cuda()
        d_tab[1, col] = value
        rc, got = run(d_tab)
        assert rc == 0, what
        assert (got[lo:hi] == SENTINEL).all() and (got[-SPARE:] == SENTINEL).all(), what
        assert _same_bits(got[:lo], base[:lo]) and _same_bits(got[hi:total], base[hi:total]), what
