"""audio_io.StreamResampler: audio fed in chunks gives resample_device's result for the same audio as one clip, bit for bit;
pipeline.StreamDenoiser(in_sr=, out_sr=) puts one in front of and one behind the networks."""
import warnings

import numpy as np
import pytest
import torch

import sos_amd
import stream_resample_reference as SR
from oracle import nets as onet
from oracle import wave_io as owio

pytestmark = pytest.mark.gpu

RESAMPLE_TOL = 1e-5                     # the one-clip test's tolerance (tests/test_gpu_wave_io.py)
MAX_CHUNK = 1024                        # small, so that a chunk above it goes in pieces
_cache = {}


def _ids(pair):
    return "%d-%d" % pair


def _R(pair):
    return 32769 // int(min(1.0, pair[1] / pair[0]) * 512)


def _streams(pair):
    """Per rate pair: standard-normal streams of 1, 2 R + 5 and 9 001 samples (the middle one scaled by 1e3) on the host and
    the GPU, and resample_device of each as one clip (None where it refuses the clip).  Computed once, never modified."""
    from sos_amd import audio_io
    if pair not in _cache:
        rng = np.random.default_rng(pair[0] * 7 + pair[1])
        host = [rng.standard_normal(n).astype(np.float32) * (1e3 if i == 1 else 1.0) for i, n in enumerate((1, 2 * _R(pair) + 5, 9001))]
        dev = [torch.from_numpy(x).cuda() for x in host]
        whole = {}
        for fix in (True, False):
            whole[fix] = [audio_io.resample_device(x, *pair, fix=fix) if int(x.numel() * pair[1] / pair[0]) >= 1 else None for x in dev]
        _cache[pair] = (host, dev, whole)
    return _cache[pair]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _feed(rs, streams, sizes):
    """Pushes stream s in chunks of sizes[s] (then whatever is left in one chunk), all slots interleaved call by call; every
    second chunk of slot 1 goes in as a host array.  -> per slot the list of pushed outputs."""
    at, outs, step = {s: 0 for s in streams}, {s: [] for s in streams}, 0
    while any(at[s] < streams[s].numel() for s in streams):
        chunks = {}
        for s, x in streams.items():
            if at[s] < x.numel():
                n = sizes[s][step] if step < len(sizes[s]) else x.numel() - at[s]
                c = x[at[s]:at[s] + n]
                chunks[s] = c.cpu().numpy() if s == 1 and step % 2 else c
                at[s] += c.numel()
        for s, y in rs.push(chunks).items():
            assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 1
            outs[s].append(y)
        step += 1
    return outs


@pytest.mark.parametrize("fix", [True, False], ids=["fix", "nofix"])
@pytest.mark.parametrize("pair", SR.RATE_PAIRS, ids=_ids)
def test_three_streams_in_chunks_are_resample_device_bit_for_bit(pair, fix):
    from sos_amd import audio_io
    host, dev, whole = _streams(pair)
    R = _R(pair)
    rs = audio_io.StreamResampler(3, *pair, fix=fix, max_chunk=MAX_CHUNK)
    assert rs.R == R and rs.capacity == MAX_CHUNK + 2 * R - 1
    sizes = {0: [0, 1], 1: [1, 0, R, R + 1, 3], 2: [0, 1, R, R + 1, MAX_CHUNK + 2 * R + 500, 7, 1000]}
    outs = _feed(rs, dict(enumerate(dev)), sizes)
    for s in (0, 1, 2):
        if whole[fix][s] is None:                               # one sample at a falling rate: no output sample
            with pytest.raises(ValueError, match="slot 0: Input signal length=1 is too small to resample from %d->%d" % pair):
                rs.close(s)
            with pytest.raises(ValueError, match="length=1 is too small"):
                audio_io.resample_device(dev[s], *pair, fix=fix)
            continue
        got = torch.cat(outs[s] + [rs.close([s])[s]])
        assert got.shape == whole[fix][s].shape and torch.equal(_bits(got), _bits(whole[fix][s])), (pair, fix, s)
        ref = owio.resample(host[s].astype(np.float64), *pair, fix=fix)
        err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - ref)) / np.max(np.abs(ref)))
        print(pair, "fix" if fix else "nofix", "stream", s, "peak error against the float64 oracle %.3e" % err)
        assert err < RESAMPLE_TOL
    assert rs.n_recv == [None] * 3
    # most of the long stream came out of push(): close() only holds what waits for its right wing
    assert sum(y.numel() for y in outs[2]) >= whole[fix][2].numel() - (R + 1) * max(pair[1] / pair[0], 1) - 2


def test_a_prefix_pushed_sample_by_sample():
    from sos_amd import audio_io
    pair = (48000, 14000)
    _, dev, whole = _streams(pair)
    x = dev[2]
    rs = audio_io.StreamResampler(1, *pair, max_chunk=MAX_CHUNK)
    got = [rs.push({0: x[i:i + 1]})[0] for i in range(600)]
    assert sum(y.numel() for y in got) == rs.t_done[0] > 100 and max(y.numel() for y in got) == 1
    got += [rs.push({0: x[600:]})[0], rs.close(0)[0]]
    assert torch.equal(_bits(torch.cat(got)), _bits(whole[True][2]))


def test_slots_are_independent_and_can_be_used_again():
    from sos_amd import audio_io
    pair = (44100, 14000)
    rng = np.random.default_rng(5)
    a, b, c = (torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda() for n in (3001, 2500, 1777))
    want = {k: audio_io.resample_device(v, *pair) for k, v in (("a", a), ("b", b), ("c", c))}

    def chunks(x, i):
        return x[700 * i:700 * (i + 1)]

    alone = audio_io.StreamResampler(4, *pair, max_chunk=MAX_CHUNK)
    one = [alone.push({2: chunks(a, i)})[2] for i in range(5)]
    among = audio_io.StreamResampler(4, *pair, max_chunk=MAX_CHUNK)
    three = [among.push({3: chunks(c, i), 0: chunks(b, i), 2: chunks(a, i)} if i % 2 else {2: chunks(a, i), 3: chunks(c, i), 0: chunks(b, i)})
             for i in range(5)]
    for i in range(5):                                          # the same pieces alone, among others, in any order of the call
        assert one[i].numel() > 0 and torch.equal(_bits(one[i]), _bits(three[i][2]))
    rest = among.close([3, 2, 0])
    for k, s in (("a", 2), ("b", 0), ("c", 3)):
        assert torch.equal(_bits(torch.cat([p[s] for p in three] + [rest[s]])), _bits(want[k])), k
    assert torch.equal(_bits(torch.cat(one + [alone.close(2)[2]])), _bits(want["a"]))
    # slot 2's ring still holds stream a: a new stream there starts at t = 0 and does not see it
    again = [among.push({2: c[:1000]})[2], among.push({2: c[1000:]})[2], among.close(2)[2]]
    assert torch.equal(_bits(torch.cat(again)), _bits(want["c"]))
    among.push({1: a[:900]})
    among.drop([1])
    assert among.n_recv == [None] * 4
    with pytest.raises(ValueError, match="slot 1 has no open stream"):
        among.drop(1)
    assert torch.equal(_bits(torch.cat([among.push({1: b})[1], among.close(1)[1]])), _bits(want["b"]))


def test_the_same_rate_passes_chunks_through():
    from sos_amd import audio_io
    _, dev, _ = _streams((14000, 16000))
    rs = audio_io.StreamResampler(2, 14000, 14000)
    got = [rs.push({1: dev[2][:500]})[1], rs.push({1: dev[2][500:].cpu().numpy()})[1], rs.close([1])[1]]
    assert got[2].numel() == 0 and got[1].is_cuda and torch.equal(torch.cat(got), dev[2])


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
    pair = (48000, 14000)
    host, dev, whole = _streams(pair)
    x = dev[2]

    def session(slots):
        rs = audio_io.StreamResampler(slots, *pair, max_chunk=MAX_CHUNK)
        got = [rs.push({0: x[i:i + 2500], 1: host[2][i:i + 2500]}) for i in range(0, 9001, 2500)]
        rest = rs.close([0, 1])
        return [torch.cat([g[s] for g in got] + [rest[s]]) for s in (0, 1)]

    session(2)                                                  # filter table, code object, pinned staging
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = session(2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for y in outs:
        assert torch.equal(_bits(y), _bits(whole[True][2]))
    few, many = audio_io.StreamResampler(2, *pair), audio_io.StreamResampler(64, *pair)
    w2 = _sync_warnings(lambda: few.push({s: x[:4800] for s in range(2)}))
    w64 = _sync_warnings(lambda: many.push({s: x[:4800] for s in range(64)}))
    print(f"synchronisation warnings of one push: 2 slots: {w2}, 64 slots: {w64}")
    assert w2 == w64 == 0


def test_refusals_come_before_any_launch():
    from sos_amd import _lib, audio_io
    pair = (48000, 14000)
    host, dev, _ = _streams(pair)
    x = dev[2]
    rs = audio_io.StreamResampler(2, *pair, max_chunk=MAX_CHUNK)
    rs.push({0: x[:1]})                                         # a stream too short to resample; the filter table is up
    h = _lib.lib()
    good = np.asarray([[0, 0, 0, 0, 0, 0]], dtype=np.int64)
    d_good = torch.from_numpy(good).cuda()                      # the device table is never the corrupted one (and never read)
    out = torch.empty(64, dtype=torch.float32, device="cuda")
    cap = rs.capacity
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for slots in (0, 65536):
            with pytest.raises(ValueError, match="slots"):
                audio_io.StreamResampler(slots, *pair)
        with pytest.raises(ValueError, match="res_type 'kaiser_fast' is not supported"):
            audio_io.StreamResampler(1, *pair, res_type="kaiser_fast")
        with pytest.raises(ValueError, match="too small for the filter's 512-point table"):
            audio_io.StreamResampler(1, 14000 * 600, 14000)     # index_step = int(512 / 600) = 0
        with pytest.raises(ValueError, match="max_chunk"):
            audio_io.StreamResampler(1, *pair, max_chunk=0)
        for slot in (2, -1, "0"):
            with pytest.raises(ValueError, match="unknown slot"):
                rs.push({slot: x})
        for chunk in (x[None], x.double(), host[2].astype(np.float64), [0.0] * 10):
            with pytest.raises(ValueError, match="1-D float32"):
                rs.push({1: chunk})
        assert rs.n_recv == [1, None]                           # nothing was opened
        for call in (rs.close, rs.drop):
            with pytest.raises(ValueError, match="slot 1 has no open stream"):
                call([0, 1])
            with pytest.raises(ValueError, match="named twice"):
                call([0, 0])
        with pytest.raises(ValueError, match="slot 0: Input signal length=1 is too small to resample from 48000->14000"):
            rs.close(0)
        with pytest.raises(ValueError, match="slot 0 has no open stream"):
            rs.close(0)
        # the ABI refuses a bad HOST row with SOS_EINVAL and names it; rows {slot, t_lo, t_hi, n_in, n_valid, output offset}
        ok = [0, 0, 10, 1000, 10, 0]
        for rows, told in (([ok, [2, 0, 10, 1000, 10, 10]], "row 1 names a slot outside the slots"),
                           ([[0, 11, 10, 1000, 10, 0]], "row 0 has outputs that are no range"),
                           ([ok, [1, 0, 10, 1000, 292, 10]], "row 1 has a length or a number of valid outputs"),
                           ([[0, 0, 10, -1, 0, 0]], "row 0 has a length"),
                           ([[0, 0, 10, 1000, 10, 55]], "row 0 writes outside the output buffer"),
                           ([[1, 0, 10, 1000, 10, -1]], "row 0 writes outside the output buffer"),
                           ([ok, [1, 0, 10, cap + 1, 10, 10]], "row 1 reads samples its ring does not hold"),
                           ([ok, [1, 0, 10, 1000, 10, 10], [0, 10, 20, 1000, 20, 20]], "row 2 names slot 0, which an earlier row")):
            tab = np.asarray(rows, dtype=np.int64)
            rc = h.sos_stream_resample_f32(_lib.ptr(rs.ring), 2, cap, _lib.ptr(d_good), tab.ctypes.data, len(rows), rs.ratio,
                                           _lib.ptr(rs.win), rs.win.numel(), rs.num_table, _lib.ptr(out), out.numel(), None)
            assert rc == -22 and told in h.sos_last_error().decode(), (rows, rc, h.sos_last_error())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # the slot is free again and streams as ever
    got = torch.cat([rs.push({0: x})[0], rs.close(0)[0]])
    assert torch.equal(_bits(got), _bits(_streams(pair)[2][True][2]))


# ---- pipeline.StreamDenoiser(in_sr=, out_sr=): geometry, networks and one wave of tests/test_gpu_stream_denoiser.py
HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SECONDS = dict(window_seconds=CORE / 14000, context_seconds=CONTEXT / 14000)
N_LONG = 3 * CORE + 5 * HOP + 77
N_16K = N_LONG * 16 // 14 + 3


@pytest.fixture(scope="module")
def nets():
    from sos_amd.common import MyConfig
    from sos_amd.denoiser import networks as jnet
    from sos_amd.detector import networks as dnet
    det = dnet.get_network()
    det.load_state_dict(onet.closed_form_state(onet.detector_spec(), seed=1))
    jm = jnet.get_network(MyConfig())
    jm.load_state_dict(onet.closed_form_state(onet.joint_spec(), seed=2))
    return det.cuda().eval(), jm.cuda().eval()


@pytest.fixture(scope="module")
def wave16():
    """Synthetic noisy speech taken as a 16 kHz stream, on the GPU.  Never modified."""
    from sos_amd.dataset import synth_batch
    parts = synth_batch(710, (N_16K + 27999) // 28000)["mixed"]
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(list(parts))[:N_16K])).cuda()


def _session(sd, x, sizes):
    at, got, i = 0, [], 0
    while at < x.numel():
        n = sizes[i % len(sizes)]
        got.append(sd.push({0: x[at:at + n]})[0])
        at, i = at + n, i + 1
    got.append(sd.close([0])[0])
    return torch.cat(got)


@pytest.fixture(scope="module")
def plain(nets, wave16):
    """The existing path: resample_device to 14 kHz, a StreamDenoiser without the keywords (every window alone, fp16).  -> (the
    14 kHz input, its denoised stream)."""
    from sos_amd import audio_io, pipeline
    det, jm = nets
    x14 = audio_io.resample_device(wave16, 16000, 14000)
    sos_amd.set_precision("fp16")
    try:
        S = _session(pipeline.StreamDenoiser(det, jm, 1, max_batch=1, **SECONDS), x14, [4000])
    finally:
        sos_amd.set_precision("bf16")
    assert bool(torch.isfinite(S).all()) and S.numel() == x14.numel() // HOP * HOP
    return x14, S


@pytest.mark.parametrize("case", ["in and out", "in only", "neither"])
def test_stream_denoiser_at_the_devices_rate(nets, wave16, plain, case):
    from sos_amd import audio_io, pipeline
    det, jm = nets
    x14, S = plain
    rates = {"in and out": dict(in_sr=16000, out_sr=16000), "in only": dict(in_sr=16000), "neither": dict(in_sr=None, out_sr=None)}[case]
    sos_amd.set_precision("fp16")
    try:
        sd = pipeline.StreamDenoiser(det, jm, 1, max_batch=1, **SECONDS, **rates)
        got = _session(sd, x14 if case == "neither" else wave16, [5000, 1, 0, 7001, 333])
    finally:
        sos_amd.set_precision("bf16")
    want = audio_io.resample_device(S, 14000, 16000) if case == "in and out" else S
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    assert sd.plans == [None] and all(rs is None or rs.n_recv == [None] for rs in (sd.rs_in, sd.rs_out))
