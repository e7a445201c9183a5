"""sos_ragged_mix_f32 / tools.add_signals_ragged on the MI355X against the float64 restatement tests/mix_reference.py.
Bounds (stated against the restatement, never against the kernel; tests/test_mix_reference.py asserts the preconditions):
  outputs   |got - ref| <= 6e-7 max(peak_out, tiny), peak_out = the reference's max |mixed| (3e-7 at norm 0.5, the bound of
            tests/test_gpu_frontend.py on sos_add_signals_f32): four f32 roundings (gain, multiply-add, inv, multiply) of about
            6e-8 each, relative to the peak;
  Es, Ez    relative error <= n 2^-52: two orders of adding n non-negative f64 terms (f32 squares are exact in f64);
  gain, inv within 2^-23 relative: one f32 rounding plus the energies' error;
  peak      within 6e-7 of the reference's peak (the output bound, on the mix before normalisation).
The output bound counts roundings relative to the peak of the sum, so every input keeps its two terms within
mix_reference.MAX_SPREAD peaks of it (asserted on the reference before each comparison; a two-sample clip whose terms cancel to
1/35 of themselves measured 1.2e-6 and was replaced by another seed).  No sample and no clip is left out of a comparison.
Every clip is at most 3 MIX_CHUNK + 3 samples or 2 s."""
import numpy as np
import pytest
import torch

import mix_reference as R

pytestmark = pytest.mark.gpu
OUT_KEYS = ("mixed", "clean", "noise")


def _chunk():
    from sos_amd import _lib as L
    return L.MIX_CHUNK


def _run(signals, noises, snr, **kw):
    """add_signals_ragged -> per clip (dict of host arrays, detail dict)."""
    from sos_amd import ragged, tools
    mixed, clean, noise, detail = tools.add_signals_ragged(signals, noises, snr, return_detail=True, **kw)
    host = ragged.download(mixed + clean + noise)
    B = len(mixed)
    return [(dict(mixed=host[i], clean=host[B + i], noise=host[2 * B + i]), detail[i]) for i in range(B)]


def _agree(got, det, ref, what):
    n = len(ref["mixed"])
    assert ref["spread"] <= R.MAX_SPREAD, (what, ref["spread"])              # the inputs' precondition (mix_reference.mix)
    peak_out = max(float(np.max(np.abs(ref["mixed"]))), R.TINY)
    worst = 0.0
    for k in OUT_KEYS:
        assert got[k].dtype == np.float32 and got[k].shape == (n,), (what, k)
        worst = max(worst, float(np.max(np.abs(got[k].astype(np.float64) - ref[k]))))
    e_rel = max(abs(det["signal_energy"] - ref["Es"]) / max(ref["Es"], R.TINY), abs(det["noise_energy"] - ref["Ez"]) / max(ref["Ez"], R.TINY))
    f_rel = max(abs(det["gain"] - ref["gain"]) / ref["gain"], abs(det["inv"] - ref["inv"]) / ref["inv"])
    p_rel = abs(det["peak"] - ref["peak"]) / max(ref["peak"], R.TINY)
    print(f"MIX {what}: n {n} outputs {worst / peak_out:.2e} of the peak (bound {R.OUT_TOL:.0e}), energies {e_rel / 2.0 ** -52:.2f} "
          f"x 2^-52 (bound {n}), gain/inv {f_rel / 2.0 ** -23:.3f} x 2^-23 (bound 1), peak {p_rel:.2e} (bound {R.OUT_TOL:.0e})")
    for k in OUT_KEYS:
        assert np.all(np.abs(got[k].astype(np.float64) - ref[k]) <= R.OUT_TOL * peak_out), (what, k)
    assert abs(det["signal_energy"] - ref["Es"]) <= n * 2.0 ** -52 * ref["Es"], what
    assert abs(det["noise_energy"] - ref["Ez"]) <= n * 2.0 ** -52 * ref["Ez"], what
    assert abs(det["gain"] - ref["gain"]) <= R.FACTOR_TOL * ref["gain"], what
    assert abs(det["inv"] - ref["inv"]) <= R.FACTOR_TOL * ref["inv"], what
    assert abs(det["peak"] - ref["peak"]) <= R.OUT_TOL * max(ref["peak"], R.TINY), what
    assert det["gain"] == float(np.float32(det["gain"])) and det["inv"] == float(np.float32(det["inv"]))     # the f32 factors


def _same(a, b):
    return all(np.array_equal(a[0][k], b[0][k]) for k in OUT_KEYS) and a[1] == b[1]


@pytest.mark.parametrize("reverse", [False, True], ids=["in-order", "reversed"])
def test_chunk_and_vector_edges(reverse):
    C = _chunk()
    clips, rec, snrs, starts = R.edge_case(C)
    assert [len(c) for c in clips] == [1, 2, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, 3 * C]
    order = list(range(len(clips)))[::-1] if reverse else list(range(len(clips)))
    res = _run([clips[i] for i in order], [rec], [snrs[i] for i in order], noise_index=[0] * len(order),
               starts=[starts[i] for i in order])
    for (got, det), i in zip(res, order):
        _agree(got, det, R.mix(clips[i], rec, snrs[i], start=starts[i]), f"edge clip {i}{' reversed' if reverse else ''}")


def test_zero_fill_of_a_short_crop():
    C = _chunk()
    rng = np.random.default_rng(41)
    n = 2 * C + 3
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    rec = (0.1 * rng.standard_normal(n + 5)).astype(np.float32)
    counts = [0, 1, n - 1, n, C, C + 1, 10 * n]
    starts = [0, 0, 0, 0, 2, 1, 10]                                          # the last: 10 n asked for, n - 5 there
    res = _run([x] * len(counts), [rec], 7.0, noise_index=[0] * len(counts), starts=starts, counts=counts)
    for (got, det), st, cnt in zip(res, starts, counts):
        ref = R.mix(x, rec, 7.0, start=st, count=cnt)
        nz = R.crop(len(rec), st, cnt, n)[1]
        assert nz == (n - 5 if cnt == 10 * n else cnt)
        _agree(got, det, ref, f"crop of {nz}")
        assert np.all(got["noise"][nz:] == 0) and np.array_equal(got["mixed"][nz:], got["clean"][nz:])
        if nz == 0:
            assert det["gain"] == 1.0 and det["noise_energy"] == 0.0


def test_degenerate_clips():
    C = _chunk()
    rng = np.random.default_rng(43)
    n = C + 7
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    z = (0.1 * rng.standard_normal(n)).astype(np.float32)
    zero = np.zeros(n, np.float32)
    sx, sz, sbits, sratio = R.silenced_case()
    sig, noi = [zero, x, zero, sx], [z, zero, zero, sz]
    bits, ratios = [None, None, None, sbits], [None, None, None, sratio]
    res = _run(sig, noi, -10.0, bits=bits, ratios=ratios)
    for k, ((got, det), what) in enumerate(zip(res, ("zero signal", "zero noise", "both zero", "silenced by its bits"))):
        _agree(got, det, R.mix(sig[k], noi[k], -10.0, bits=bits[k], ratio=ratios[k]), what)
    (g0, d0), (g1, d1), (g2, d2), (g3, d3) = res
    assert d0["gain"] == 1.0 and np.array_equal(g0["noise"], z * np.float32(d0["inv"])) and np.all(g0["clean"] == 0)
    assert d1["gain"] == 1.0 and np.all(g1["noise"] == 0) and np.array_equal(g1["mixed"], g1["clean"])
    assert d2["inv"] == 1.0 and d2["gain"] == 1.0 and all(np.all(g2[k] == 0) for k in OUT_KEYS)
    assert d3["signal_energy"] == 0.0 and d3["gain"] == 1.0 and np.all(g3["clean"] == 0)
    assert np.array_equal(g3["noise"], sz * np.float32(d3["inv"]))
    for norm in (None, 0):
        (got, det), = _run([x], [z], 7.0, norm=norm)
        _agree(got, det, R.mix(x, z, 7.0, norm=norm), f"norm={norm}")
        assert det["inv"] == 1.0


def test_frame_decisions_silence_the_clip_with_the_mask_of_bits_to_mask():
    from sos_amd import tools
    clips, noises, snrs, bits, ratios = R.speech_case()
    res = _run(clips, noises, snrs, bits=bits, ratios=ratios)
    dev = tools.add_signals_ragged(clips, noises, snrs, bits=bits, ratios=ratios, return_detail=True)
    for i, (got, det) in enumerate(res):
        _agree(got, det, R.mix(clips[i], noises[i], snrs[i], bits=bits[i], ratio=ratios[i]), f"speech clip {i}")
        x = torch.from_numpy(clips[i]).cuda()
        if bits[i] is not None:
            mask = tools.bits_to_mask_batch(torch.from_numpy(bits[i]).cuda()[None], ratios[i], len(clips[i]))[0]
            assert 0 < float(mask.sum()) < len(clips[i])
            x = x * (1 - mask)
        assert torch.equal(dev[1][i], x * torch.tensor(det["inv"], dtype=torch.float32, device="cuda")), i


def _independence_inputs():
    C = _chunk()
    clips, rec, snrs, starts = R.edge_case(C)
    cases = [dict(signal=c, noise=rec, snr=s, start=st, bits=None, ratio=None) for c, s, st in zip(clips, snrs, starts)]
    clips, noises, snrs, bits, ratios = R.speech_case()
    cases += [dict(signal=c, noise=z, snr=s, start=0, bits=b, ratio=r) for c, z, s, b, r in zip(clips, noises, snrs, bits, ratios)]
    return cases


def _batch(cases):
    return _run([c["signal"] for c in cases], [c["noise"] for c in cases], [c["snr"] for c in cases],
                starts=[c["start"] for c in cases], bits=[c["bits"] for c in cases], ratios=[c["ratio"] for c in cases])


def test_a_clip_has_the_same_bits_alone_from_gpu_tensors_and_behind_a_dummy_clip():
    cases = _independence_inputs()
    together = _batch(cases)
    dummy = dict(signal=np.asarray([0.1, -0.2, 0.05], np.float32), noise=np.ones(3, np.float32), snr=0.0, start=0, bits=None,
                 ratio=None)
    for i, c in enumerate(cases):
        alone, = _batch([c])
        tensor = dict(c, signal=torch.from_numpy(c["signal"]).cuda(), noise=torch.from_numpy(c["noise"]).cuda())
        if c["bits"] is not None:
            tensor["bits"] = torch.from_numpy(c["bits"]).cuda()
        from_gpu, = _batch([tensor])
        behind = _batch([dummy, c])[1]
        assert _same(alone, together[i]) and _same(alone, from_gpu) and _same(alone, behind), i


def test_chunks_of_max_clips_give_the_bits_of_one_launch_sequence(monkeypatch):
    cases = _independence_inputs()
    want = _batch(cases)
    monkeypatch.setattr("sos_amd.ragged.MAX_CLIPS", 3)
    got = _batch(cases)
    assert len(got) == len(want) == 14 and all(_same(a, b) for a, b in zip(got, want))


def test_device_entries_that_disagree_with_the_host_get_status_minus_one():
    """The kernels follow the DEVICE tables and parameters: clip 1's entry is changed on the device after the host's checks so
    that it leaves the buffers (or the rules).  It gets status -1 and nothing of it is written; the others come out right.  No
    fault is provoked: the kernel's own bounds rule refuses the clip."""
    from sos_amd import _lib as L
    from sos_amd import ragged
    h = L.lib()
    C = _chunk()
    rng = np.random.default_rng(47)
    lens, nb = [C + 5, 2 * C + 1, 700], [0, 9, 0]
    xs = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    rec = (0.1 * rng.standard_normal(3 * C)).astype(np.float32)
    bits1 = np.asarray([1, 1, 0, 0, 1, 1, 1, 0, 1], np.uint8)
    tab = ragged.clip_table(lens, nb)
    ntab = np.asarray([[5, lens[0]], [1, lens[1]], [9, 600]], dtype=np.int64)
    par = np.asarray([[3.0, 0.0], [0.0, lens[1] / 9.0], [-10.0, 0.0]], dtype=np.float64)
    want = [R.mix(xs[0], rec, 3.0, start=5), None, R.mix(xs[2], rec, -10.0, start=9, count=600)]
    total = sum(lens)
    flat = torch.from_numpy(np.concatenate(xs + [np.zeros(1, np.float32)])).cuda()
    d_rec, d_bits = torch.from_numpy(rec).cuda(), torch.from_numpy(bits1).cuda()
    need = h.sos_ragged_mix_workspace_bytes(tab.ctypes.data, 3)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    edits = (("sample offset", "tab", 0, total - lens[1] + 1), ("samples", "tab", 1, total + 1), ("frame offset", "tab", 2, 1),
             ("crop longer than the clip", "ntab", 1, lens[1] + 1), ("crop past the noise", "ntab", 0, len(rec) - lens[1] + 1),
             ("negative crop offset", "ntab", 0, -1), ("ratio", "par", 1, 1.0), ("snr", "par", 0, float("inf")))
    for what, which, col, value in edits:
        d_tab, d_ntab, d_par = torch.from_numpy(tab).cuda(), torch.from_numpy(ntab).cuda(), torch.from_numpy(par).cuda()
        dict(tab=d_tab, ntab=d_ntab, par=d_par)[which][1, col] = value
        outs = [torch.full((total,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
        out = torch.full((3, 6), 5.0, dtype=torch.float64, device="cuda")
        rc = h.sos_ragged_mix_f32(L.ptr(flat), L.ptr(d_tab), tab.ctypes.data, 3, L.ptr(d_rec), len(rec), L.ptr(d_ntab),
                                  ntab.ctypes.data, L.ptr(d_bits), L.ptr(d_par), par.ctypes.data, 0.5, L.ptr(ws), need,
                                  L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(out), L.stream_ptr())
        assert rc == 0, (what, h.sos_last_error().decode())
        o = out.cpu().numpy()
        host = [t.cpu().numpy() for t in outs]
        assert o[1, 5] == -1 and o[0, 5] == 0 and o[2, 5] == 0, (what, o)
        for arr in host:
            assert np.all(arr[lens[0]:lens[0] + lens[1]] == 7.0), what       # nothing written for the refused clip
        for i, off in ((0, 0), (2, lens[0] + lens[1])):
            got = {k: host[j][off:off + lens[i]] for j, k in enumerate(OUT_KEYS)}
            det = dict(signal_energy=o[i, 0], noise_energy=o[i, 1], gain=o[i, 2], peak=o[i, 3], inv=o[i, 4])
            _agree(got, det, want[i], f"{what}: clip {i}")
    # the sound tables: clip 1 is mixed too
    outs = [torch.full((total,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    out = torch.full((3, 6), 5.0, dtype=torch.float64, device="cuda")
    d_tab, d_ntab, d_par = torch.from_numpy(tab).cuda(), torch.from_numpy(ntab).cuda(), torch.from_numpy(par).cuda()
    assert h.sos_ragged_mix_f32(L.ptr(flat), L.ptr(d_tab), tab.ctypes.data, 3, L.ptr(d_rec), len(rec), L.ptr(d_ntab),
                                ntab.ctypes.data, L.ptr(d_bits), L.ptr(d_par), par.ctypes.data, 0.5, L.ptr(ws), need,
                                L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(out), L.stream_ptr()) == 0
    o = out.cpu().numpy()
    assert np.all(o[:, 5] == 0)
    got = {k: outs[j].cpu().numpy()[lens[0]:lens[0] + lens[1]] for j, k in enumerate(OUT_KEYS)}
    _agree(got, dict(signal_energy=o[1, 0], noise_energy=o[1, 1], gain=o[1, 2], peak=o[1, 3], inv=o[1, 4]),
           R.mix(xs[1], rec, 0.0, start=1, bits=bits1, ratio=lens[1] / 9.0), "sound tables: clip 1")


def test_a_refused_clip_is_reported_by_number(monkeypatch):
    """tools.add_signals_ragged raises on a status of -1, naming the clip (here the ratio goes up as 1 behind the checks)."""
    from sos_amd import ragged, tools
    x = np.ones(50, np.float32)
    real = ragged.upload

    def upload(host, device):
        if host.dtype == np.float64 and host.shape[1:] == (2,):
            host = host.copy()
            host[1, 1] = 1.0
        return real(host, device)
    monkeypatch.setattr(ragged, "upload", upload)
    with pytest.raises(RuntimeError, match="clip 1"):
        tools.add_signals_ragged([x, x], [x, x], 3.0, bits=[np.ones(2, np.uint8)] * 2, ratios=25.0)
