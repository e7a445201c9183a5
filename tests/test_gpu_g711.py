"""G.711 on the GPU: sos_g711_planes_batch_f32 / sos_g711_encode_batch / sos_g711_to_mono_f32 (csrc/pcm_io.hip, csrc/wave_io.hip,
the rule in csrc/pcm_core.h) through audio_io and recordings, against tests/g711_reference.py (itself held against audioop in
tests/test_g711_reference.py).  The rule is whole-number arithmetic on a value that is exact in float32, so EVERY comparison is
equality of bits, bytes and counts: there is no tolerance in this file.  The domain is small enough to cover whole: all 256 codes
in, all 65 536 s16 values (and what lies between and beyond them) out.
Shapes: files of 1, 3, 4, 5, 255, 256 and 1025 frames with 1, 2 and 3 channels in ONE launch -- after the first file of one
frame every later file starts off a dword on the code side and most planes off 16 bytes; 1025 x 3 spans several workgroups."""
import ctypes as C

import numpy as np
import pytest
import torch

import g711_reference as G
import pcm_reference as R
from oracle import nets as onet

pytestmark = pytest.mark.gpu
LAWS = ("alaw", "ulaw")
SHAPES = [(n, c) for c in (1, 2, 3) for n in (1, 3, 4, 5, 255, 256, 1025)]       # 21 files, 9294 codes
SENTINEL = 0xA5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ decode
@pytest.fixture(scope="module")
def code_files():
    """Every code byte many times over, at every position of a dword and in every channel: 7 is coprime to 256."""
    total = sum(n * c for n, c in SHAPES)
    flat = ((np.arange(total, dtype=np.int64) * 7 + 3) % 256).astype(np.uint8)
    assert len(set(flat.tolist())) == 256
    files, at = [], 0
    for n, c in SHAPES:
        files.append(flat[at:at + n * c].reshape(n, c))
        at += n * c
    return files


@pytest.mark.parametrize("law", LAWS)
def test_decode_planes_are_the_reference_bit_for_bit(law, code_files):
    from sos_amd import audio_io
    ys = audio_io.decode_planes_batch_device(code_files, [law] * len(code_files))
    base = ys[0].untyped_storage().data_ptr()
    assert sum(y.storage_offset() % 4 != 0 for y in ys) >= 10                     # planes off 16 bytes are among them
    for a, y in zip(code_files, ys):
        assert y.shape == (a.shape[1], a.shape[0]) and y.dtype == torch.float32 and y.untyped_storage().data_ptr() == base
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(G.decode(a, law))), (law, a.shape)


@pytest.mark.parametrize("law", LAWS)
def test_mono_is_the_mean_expression_on_the_reference_planes(law, code_files):
    from sos_amd import audio_io
    for a in code_files:
        mono = audio_io.pcm_to_mono_device(torch.from_numpy(a).cuda(), law)
        assert mono.shape == (a.shape[0],) and np.array_equal(_bits(mono.cpu().numpy()), _bits(G.mono(a, law))), (law, a.shape)


def test_decode_of_both_laws_and_u8_in_one_call_keeps_them_apart(code_files):
    """The three one-byte formats share a dtype: each goes through its own rule."""
    from sos_amd import audio_io
    kinds = [("alaw", "u8", "ulaw")[j % 3] for j in range(len(code_files))]
    ys = audio_io.decode_planes_batch_device(code_files, kinds)
    for a, k, y in zip(code_files, kinds, ys):
        want = R.decode(a, k) if k == "u8" else G.decode(a, k)
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(want)), (k, a.shape)


# ------------------------------------------------------------------------------------------------ encode
@pytest.fixture(scope="module")
def plane_files():
    """k / 32768 for every s16 k, the s16 rule's edge values and a seeded block over [-1.5, 1.5]: 69 655 samples, an odd number.
    Files: one channel at output 0; one channel after it, at an odd output offset and a plane off 16 bytes; two channels,
    cropped; three channels, zero-filled past the plane."""
    rng = np.random.default_rng(61)
    x = np.concatenate([(np.arange(-32768, 32768) / 32768.0).astype(np.float32), R.edge_values("s16"),
                        rng.uniform(-1.5, 1.5, size=4097).astype(np.float32)])
    n = x.size
    assert n % 2 == 1
    planes = [x.reshape(1, n), x[::-1].copy().reshape(1, n), x[:2 * (n // 2)].reshape(2, n // 2), x[1:1 + 3 * (n // 3)].reshape(3, n // 3)]
    frames = [n, n, n // 2 - 5, n // 3 + 37]
    return planes, frames


@pytest.mark.parametrize("law", LAWS)
def test_encode_bytes_and_counts_are_the_reference(law, plane_files):
    from sos_amd import audio_io
    planes, frames = plane_files
    ref = [G.encode(p, law, f) for p, f in zip(planes, frames)]
    dev = [torch.from_numpy(p).cuda() for p in planes]
    data, offsets, clipped = audio_io.encode_batch_device(dev, law, frames=frames)
    assert data.dtype == torch.uint8 and np.array_equal(offsets, np.cumsum([0] + [f * p.shape[0] for p, f in zip(planes, frames)]))
    got = data.cpu().numpy()
    for j, (want, _) in enumerate(ref):
        mine = got[offsets[j]:offsets[j + 1]]
        differ = np.flatnonzero(mine != np.frombuffer(want, dtype=np.uint8))
        assert differ.size == 0, (law, j, differ[:8], mine[differ[:8]])
    print(law, "clipped", clipped.cpu().tolist(), "reference", [r[1] for r in ref])
    assert clipped.cpu().tolist() == [r[1] for r in ref] and min(r[1] for r in ref) > 0
    assert torch.equal(clipped, audio_io.encode_batch_device(dev, "s16", frames=frames)[2])      # exactly what 's16' counts
    tail = got[offsets[3]:offsets[4]].reshape(frames[3], 3)[planes[3].shape[1]:]
    assert tail.shape == (37, 3) and np.all(tail == G.SILENCE[law])               # the zero-fill is silence, never byte 0
    again = audio_io.encode_batch_device(dev, law, frames=frames)                 # two calls: identical bytes and counts
    assert torch.equal(again[0], data) and torch.equal(again[2], clipped)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("law", LAWS)
def test_encode_leaves_the_sentinels_wherever_the_output_starts(law, lead):
    """The entry point itself, the output between sentinel bytes and starting `lead` bytes past a 256-byte boundary."""
    from sos_amd import _lib as L
    from sos_amd import audio_io
    rng = np.random.default_rng(67)
    planes = [rng.uniform(-1.2, 1.2, size=(c, n)).astype(np.float32) for n, c in SHAPES]
    frames = np.asarray([(max(n - 1 - n // 3, 0), n, n + 3 + n // 5)[k % 3] for k, (n, _) in enumerate(SHAPES)], dtype=np.int64)
    ref = [G.encode(p, law, f) for p, f in zip(planes, frames)]
    ch, avail = np.asarray([c for _, c in SHAPES], dtype=np.int64), np.asarray([n for n, _ in SHAPES], dtype=np.int64)
    src, dst = np.cumsum(ch * avail) - ch * avail, np.cumsum(ch * frames) - ch * frames
    tab = np.ascontiguousarray(np.stack([src, avail, ch, frames, dst], axis=1), dtype=np.int64)
    flat = torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).cuda()
    nbytes, pad = int((ch * frames).sum()), 256
    out = torch.full((pad + lead + nbytes + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    counts = torch.full((len(planes) + 2,), -9, dtype=torch.int64, device="cuda")
    rc = L.lib().sos_g711_encode_batch(L.ptr(flat), L.ptr(torch.from_numpy(tab).cuda()), tab.ctypes.data_as(C.c_void_p), len(planes),
                                       audio_io.G711[law][0], L.ptr(out[pad + lead:]), L.ptr(counts[1:]), L.stream_ptr())
    assert rc == 0, L.lib().sos_last_error()
    host, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert np.all(host[:pad + lead] == SENTINEL) and np.all(host[pad + lead + nbytes:] == SENTINEL), "encode wrote outside its output"
    assert host[pad + lead:pad + lead + nbytes].tobytes() == b"".join(r[0] for r in ref)
    assert counts.tolist() == [-9] + [r[1] for r in ref] + [-9]


# ------------------------------------------------------------------------------------------------ chunks of a live leg
@pytest.mark.parametrize("law", LAWS)
def test_chunks_of_160_samples_are_the_whole_signal(law):
    """20 ms packets at 8 kHz, and a last short one: the rule has no state."""
    from sos_amd import audio_io
    rng = np.random.default_rng(71)
    x = np.concatenate([rng.uniform(-1.1, 1.1, size=1600), R.edge_values("s16")]).astype(np.float32)      # 1622 = 10 x 160 + 22
    want, count = G.encode(x.reshape(1, -1), law)
    dev = torch.from_numpy(x).cuda()
    whole, clipped = audio_io.g711_encode_device(dev, law)
    assert whole.cpu().numpy().tobytes() == want and clipped.cpu().tolist() == [count]
    parts = [audio_io.g711_encode_device(dev[i:i + 160], law) for i in range(0, x.size, 160)]
    assert torch.equal(torch.cat([p[0] for p in parts]), whole) and sum(int(p[1]) for p in parts) == count
    planes = G.decode(np.frombuffer(want, dtype=np.uint8).reshape(-1, 1), law)[0]
    assert np.array_equal(_bits(audio_io.g711_decode_device(whole, law).cpu().numpy()), _bits(planes))
    on_device = torch.cat([audio_io.g711_decode_device(p[0], law) for p in parts])               # codes that stayed in HBM
    from_host = torch.cat([audio_io.g711_decode_device(want[i:i + 160], law) for i in range(0, len(want), 160)])   # payload bytes
    assert np.array_equal(_bits(on_device.cpu().numpy()), _bits(planes)) and torch.equal(on_device, from_host)


# ------------------------------------------------------------------------------------------------ recordings end to end
SECONDS = dict(window_seconds=2.0, context_seconds=0.5)
# name, rate, channels, format, frames: MIN_FRAMES = 65 STFT frames of hop 158 are 10 112 samples at 14 kHz, 5 779 at 8 kHz
SPECS = (("leg", 8000, 1, "ulaw", 6000), ("pair", 8000, 2, "alaw", 6001), ("pcm", 14000, 1, "s16", 10500))


@pytest.fixture(autouse=True)
def _parity_mode():
    import sos_amd
    sos_amd.set_precision("bf16x3")
    try:
        yield
    finally:
        sos_amd.set_precision("bf16")


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


def _encode(planes, fmt, frames=None):
    return G.encode(planes, fmt, frames) if fmt in G.TAG else R.encode(planes, fmt, frames)


def _container(data, fmt, channels, rate):
    return G.container(data, fmt, channels, rate) if fmt in G.TAG else R.container(data, fmt, channels, rate)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root, out = tmp_path_factory.mktemp("g711_in"), []
    for i, (name, rate, ch, fmt, n) in enumerate(SPECS):
        rng = np.random.default_rng(73 + i)
        t = np.arange(n) / rate
        planes = np.stack([0.3 * np.sin(2 * np.pi * (300 + 70 * c) * t) * (0.2 + (np.sin(2 * np.pi * 2.3 * t + c) > -0.4))
                           + 0.02 * rng.standard_normal(n) for c in range(ch)]).astype(np.float32)
        data, _ = _encode(planes, fmt)
        path = root / (name + ".wav")
        path.write_bytes(_container(data, fmt, ch, rate))
        out.append(dict(name=name, path=str(path), rate=rate, channels=ch, fmt=fmt, frames=n, data=data))
    return out


def _stored_planes(f):
    """What the file holds, as the reference decodes it: (channels, frames) float32."""
    if f["fmt"] in G.TAG:
        return G.decode(np.frombuffer(f["data"], dtype=np.uint8).reshape(-1, f["channels"]), f["fmt"])
    return R.decode(R.unpack(f["data"], f["fmt"], f["channels"]), f["fmt"])


@pytest.fixture(scope="module")
def one_call(nets, files, tmp_path_factory):
    """denoise_recordings over the three files, and the same chain through the public pieces from the reference's decode (to 14 kHz,
    ONE denoise_long over all channels, back): computed once and left unchanged."""
    import sos_amd
    from sos_amd import audio_io, pipeline, recordings, windows
    out_dir = tmp_path_factory.mktemp("g711_out")
    sos_amd.set_precision("bf16x3")
    try:
        res = recordings.denoise_recordings(nets[0], nets[1], [f["path"] for f in files], str(out_dir), suffix="_dn", **SECONDS)
        owner = [f for f in files for _ in range(f["channels"])]
        clips = [torch.from_numpy(np.ascontiguousarray(row)).cuda() for f in files for row in _stored_planes(f)]
        idx = [k for k, f in enumerate(owner) if f["rate"] == 8000]
        for k, y in zip(idx, audio_io.resample_batch_device([clips[k] for k in idx], 8000, pipeline.SR)):
            clips[k] = y
        outs = windows.denoise_long(nets[0], nets[1], clips, **SECONDS)
        for k, y in zip(idx, audio_io.resample_batch_device([outs[k] for k in idx], pipeline.SR, 8000)):
            outs[k] = y
        planes, k = {}, 0
        for f in files:
            planes[f["name"]] = np.stack([o.cpu().numpy() for o in outs[k:k + f["channels"]]])
            k += f["channels"]
    finally:
        sos_amd.set_precision("bf16")
    return res, planes


def test_load_device_reads_g711_files(files):
    from sos_amd import audio_io
    for f in files[:2]:
        codes = np.frombuffer(f["data"], dtype=np.uint8).reshape(-1, f["channels"])
        y, sr = audio_io.load_device(f["path"], sr=None)
        assert sr == 8000 and np.array_equal(_bits(y.cpu().numpy()), _bits(G.mono(codes, f["fmt"])))
    ys, srs, infos = audio_io.load_channels_batch_device([f["path"] for f in files])
    for f, y, sr, info in zip(files, ys, srs, infos):
        assert sr == f["rate"] and np.array_equal(_bits(y.cpu().numpy()), _bits(_stored_planes(f)))
    assert [(i["tag"], i["bits"]) for i in infos] == [(7, 8), (6, 8), (1, 16)]


def test_recordings_come_back_in_their_own_format(one_call, files):
    from sos_amd import audio_io
    res, planes = one_call
    for f, r in zip(files, res):
        tag, bits = (G.TAG[f["fmt"]], 8) if f["fmt"] in G.TAG else R.TAG_BITS[f["fmt"]]
        assert audio_io.wave_info(r["out_path"]) == dict(tag=tag, bits=bits, channels=f["channels"], rate=f["rate"], frames=f["frames"])
        assert (r["channels"], r["rate"], r["frames"], r["format"], r["windows"]) == (f["channels"], f["rate"], f["frames"], f["fmt"], f["channels"])
        data, clipped = _encode(planes[f["name"]], f["fmt"], f["frames"])
        with open(r["out_path"], "rb") as fp:
            assert fp.read() == _container(data, f["fmt"], f["channels"], f["rate"]), f["name"]
        assert r["clipped"] == clipped
        if f["fmt"] in G.TAG:                                                     # the networks return hop * (n // hop) samples
            codes = np.frombuffer(data, dtype=np.uint8).reshape(f["frames"], f["channels"])
            assert planes[f["name"]].shape[1] < f["frames"] and np.all(codes[planes[f["name"]].shape[1]:] == G.SILENCE[f["fmt"]])


def test_sample_format_ulaw_forces_all_three(one_call, nets, files, tmp_path):
    from sos_amd import audio_io, recordings
    _, planes = one_call
    res = recordings.denoise_recordings(nets[0], nets[1], [f["path"] for f in files], str(tmp_path), sample_format="ulaw", **SECONDS)
    for f, r in zip(files, res):
        assert r["format"] == "ulaw"
        assert audio_io.wave_info(r["out_path"]) == dict(tag=7, bits=8, channels=f["channels"], rate=f["rate"], frames=f["frames"])
        data, clipped = G.encode(planes[f["name"]], "ulaw", f["frames"])
        with open(r["out_path"], "rb") as fp:
            assert fp.read() == G.container(data, "ulaw", f["channels"], f["rate"]), f["name"]
        assert r["clipped"] == clipped
