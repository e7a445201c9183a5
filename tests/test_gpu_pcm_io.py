"""sos_pcm_planes_batch_f32 / sos_pcm_encode_batch (csrc/pcm_io.hip) and audio_io.decode_planes_batch_device /
encode_batch_device against the float64 restatement tests/pcm_reference.py.  The rule is exact in double (a float times a power
of two), so EVERY comparison below is equality of bits, bytes and counts: there is no tolerance in this file.
Shapes: files of 1, 2, 3, 4, 5, 255, 256, 257 and 1025 frames with 1, 2, 3 and 6 channels in ONE group (odd frame counts put the
plane starts off 16-byte boundaries and the s24 / u8 / s16 file starts off dwords; 1025 x 6 spans several workgroups), and one
file of 2 x 600 000 frames, past the 1024 x 256 x 4 elements one pass of the grid covers (the stride loop)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pcm_reference as R

pytestmark = pytest.mark.gpu
FRAMES = (1, 2, 3, 4, 5, 255, 256, 257, 1025)
CHANNELS = (1, 2, 3, 6)
SHAPES = [(n, c) for c in CHANNELS for n in FRAMES]            # 36 files
DECODE_FORMATS = ("s16", "s32", "f32", "u8")
ENCODE_FORMATS = ("s16", "s24", "s32", "u8", "f32")
NP_TYPE = dict(s16=np.int16, s32=np.int32, f32=np.float32, u8=np.uint8)
SENTINEL = 0xA5


def _pcm_file(n, ch, kind, rng):
    """(frames, channels) samples of a kind, the format's extreme values among them."""
    if kind == "f32":
        a = rng.uniform(-1.5, 1.5, size=(n, ch)).astype(np.float32)
        edge = R.edge_values("f32")
        if ch == 1:         # compared with the mono kernel, which sums onto +0.0: -0.0 and a NaN's payload are not its to keep
            edge = edge[~(np.isnan(edge) | ((edge == 0) & np.signbit(edge)))]
        a.reshape(-1)[::7] = edge[np.arange(a.size)[::7] % len(edge)]
        return a
    info = np.iinfo(NP_TYPE[kind])
    a = rng.integers(info.min, info.max, size=(n, ch), endpoint=True).astype(NP_TYPE[kind])
    a.reshape(-1)[::5] = np.asarray([info.min, info.max, 0, info.min + 1, info.max - 1], dtype=NP_TYPE[kind])[np.arange(a.size)[::5] % 5]
    if kind == "s32":
        a.reshape(-1)[1::9] &= ~np.int32(0xFF)                  # 24-bit samples as read_wave carries them
    return a


@pytest.fixture(scope="module")
def pcm_files():
    rng = np.random.default_rng(41)
    return {k: [_pcm_file(n, ch, k, rng) for n, ch in SHAPES] for k in DECODE_FORMATS}


def _planes_file(n, ch, fmt, rng, k):
    """(channels, n) float32 planes spread over [-1.5, 1.5] with the rule's tie and edge values among them (all 22 of them in
    every file of 22 samples or more, a rotating choice in the smaller ones)."""
    p = rng.uniform(-1.5, 1.5, size=(ch, n)).astype(np.float32)
    edge = R.edge_values(fmt)
    flat = p.reshape(-1)
    pos = np.arange(0, flat.size, 3 if flat.size >= 66 else 1)
    flat[pos] = edge[(pos // (3 if flat.size >= 66 else 1) + k) % len(edge)]
    return p


def _frames_for(k, n):
    """frames to write: below, equal to and above the available plane length, in turn."""
    return (max(n - 1 - n // 3, 0), n, n + 3 + n // 5)[k % 3]


@pytest.fixture(scope="module")
def plane_files():
    rng = np.random.default_rng(43)
    out = {}
    for fmt in ENCODE_FORMATS:
        planes = [_planes_file(n, ch, fmt, rng, k) for k, (n, ch) in enumerate(SHAPES)]
        frames = [_frames_for(k, n) for k, (n, _) in enumerate(SHAPES)]
        ref = [R.encode(p, fmt, f) for p, f in zip(planes, frames)]
        out[fmt] = dict(planes=planes, frames=frames, data=b"".join(r[0] for r in ref), clipped=[r[1] for r in ref])
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("kind", DECODE_FORMATS)
def test_decode_planes_are_the_reference_bit_for_bit(kind, pcm_files):
    from sos_amd import audio_io
    arrs = pcm_files[kind]
    ys = audio_io.decode_planes_batch_device(arrs, [kind] * len(arrs))
    base = ys[0].untyped_storage().data_ptr()
    for a, y in zip(arrs, ys):
        assert y.shape == (a.shape[1], a.shape[0]) and y.dtype == torch.float32 and y.untyped_storage().data_ptr() == base
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(R.decode(a, kind))), (kind, a.shape)
        if a.shape[1] == 1:                                     # one channel: the mono kernel's bits
            mono = audio_io.pcm_to_mono_device(torch.from_numpy(a).cuda(), kind)
            differ = np.flatnonzero(_bits(y[0].cpu().numpy()) != _bits(mono.cpu().numpy()))
            assert differ.size == 0, (kind, a.shape, differ[:8], a.reshape(-1)[differ[:8]])


def test_decode_of_mixed_formats_and_an_empty_file_in_one_call(pcm_files):
    from sos_amd import audio_io
    arrs, kinds = [], []
    for j in range(len(SHAPES)):                                # formats interleaved file by file
        kinds.append(DECODE_FORMATS[j % 4])
        arrs.append(pcm_files[kinds[-1]][j])
    arrs.insert(5, np.zeros((0, 2), np.int16))
    kinds.insert(5, "s16")
    ys = audio_io.decode_planes_batch_device(arrs, kinds)
    assert ys[5].shape == (2, 0)
    for a, k, y in zip(arrs, kinds, ys):
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(R.decode(a, k))), (k, a.shape)


def _raw_decode(arrs, kind, dev_edit=None):
    """The entry point itself over a sentinel-filled output: (out floats as uint32, rc).  dev_edit(table) corrupts the DEVICE copy."""
    from sos_amd import _lib as L
    from sos_amd import audio_io
    sizes = np.asarray([a.size for a in arrs], dtype=np.int64)
    off = np.cumsum(sizes) - sizes
    tab = np.ascontiguousarray(np.stack([off, [a.shape[0] for a in arrs], [a.shape[1] for a in arrs], off], axis=1), dtype=np.int64)
    dev = tab.copy()
    if dev_edit:
        dev_edit(dev)
    pcm = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).cuda()
    pad = 64
    out = torch.full((pad + int(sizes.sum()) + pad,), -7.0, dtype=torch.float32, device="cuda")
    rc = L.lib().sos_pcm_planes_batch_f32(L.ptr(pcm), audio_io._FMT[kind], L.ptr(torch.from_numpy(dev).cuda()),
                                          tab.ctypes.data_as(C.c_void_p), len(arrs), L.ptr(out[pad:]), L.stream_ptr())
    assert rc == 0, L.lib().sos_last_error()
    host = out.cpu().numpy()
    assert np.all(host[:pad] == -7.0) and np.all(host[-pad:] == -7.0), "decode wrote outside its output"
    return host[pad:-pad], off


def _corrupt(row, col, value):
    def edit(tab):
        tab[row, col] = value
    return edit


@pytest.mark.parametrize("col,value", [(0, 1 << 40), (0, -1), (1, 1 << 40), (1, -3), (2, 0), (2, 65), (3, 1 << 40), (3, -16)],
                         ids=["pcm-far", "pcm<0", "frames-huge", "frames<0", "channels=0", "channels=65", "out-far", "out<0"])
def test_decode_skips_a_device_row_outside_the_totals(col, value, pcm_files):
    arrs, victim = pcm_files["s16"], 16                         # 257 frames x 2 channels
    got, off = _raw_decode(arrs, "s16", _corrupt(victim, col, value))
    for j, a in enumerate(arrs):
        mine = got[off[j]:off[j] + a.size]
        if j == victim:
            assert np.all(mine == -7.0), "a row outside the totals was followed"
        else:
            assert np.array_equal(_bits(mine), _bits(R.decode(a, "s16")).reshape(-1)), j


# ------------------------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("fmt", ENCODE_FORMATS)
def test_encode_bytes_and_counts_are_the_reference(fmt, plane_files):
    from sos_amd import audio_io
    f = plane_files[fmt]
    planes = [torch.from_numpy(p).cuda() for p in f["planes"]]
    data, offsets, clipped = audio_io.encode_batch_device(planes, fmt, frames=f["frames"])
    want_off = np.cumsum([0] + [fr * p.shape[0] * R.WIDTH[fmt] for p, fr in zip(f["planes"], f["frames"])])
    assert data.dtype == torch.uint8 and np.array_equal(offsets, want_off)
    assert data.cpu().numpy().tobytes() == f["data"]
    assert clipped.cpu().tolist() == f["clipped"] and (fmt == "f32" or sum(f["clipped"]) > 0)
    again = audio_io.encode_batch_device(planes, fmt, frames=f["frames"])       # two calls: identical bytes and counts
    assert torch.equal(again[0], data) and torch.equal(again[2], clipped)
    same = audio_io.encode_batch_device(planes, fmt)                            # frames=None: the planes' own lengths
    assert same[0].cpu().numpy().tobytes() == b"".join(R.encode(p, fmt)[0] for p in f["planes"])


def _raw_encode(f, fmt, lead, dev_edit=None):
    """The entry point itself, the output between sentinel bytes and starting `lead` bytes past a 256-byte boundary:
    (bytes, counts, element offsets).  dev_edit(table) corrupts the DEVICE copy after the host's check."""
    from sos_amd import _lib as L
    from sos_amd import audio_io
    planes, frames = f["planes"], np.asarray(f["frames"], dtype=np.int64)
    ch, avail = np.asarray([p.shape[0] for p in planes], dtype=np.int64), np.asarray([p.shape[1] for p in planes], dtype=np.int64)
    src, dst = np.cumsum(ch * avail) - ch * avail, np.cumsum(ch * frames) - ch * frames
    tab = np.ascontiguousarray(np.stack([src, avail, ch, frames, dst], axis=1), dtype=np.int64)
    dev = tab.copy()
    if dev_edit:
        dev_edit(dev)
    flat = torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).cuda()
    nbytes, pad = int((ch * frames).sum()) * R.WIDTH[fmt], 256
    out = torch.full((pad + lead + nbytes + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    counts = torch.full((len(planes) + 2,), -9, dtype=torch.int64, device="cuda")
    rc = L.lib().sos_pcm_encode_batch(L.ptr(flat), L.ptr(torch.from_numpy(dev).cuda()), tab.ctypes.data_as(C.c_void_p), len(planes),
                                      audio_io.ENCODINGS[fmt][0], L.ptr(out[pad + lead:]), L.ptr(counts[1:]), L.stream_ptr())
    assert rc == 0, L.lib().sos_last_error()
    host, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert np.all(host[:pad + lead] == SENTINEL) and np.all(host[pad + lead + nbytes:] == SENTINEL), "encode wrote outside its output"
    assert counts[0] == -9 and counts[-1] == -9
    return host[pad + lead:pad + lead + nbytes], counts[1:-1], dst * R.WIDTH[fmt]


@pytest.mark.parametrize("fmt,lead", [("s16", 0), ("s16", 2), ("s16", 6), ("s24", 0), ("s24", 1), ("s24", 2), ("s24", 3), ("s32", 0),
                                      ("s32", 4), ("u8", 0), ("u8", 1), ("u8", 3), ("f32", 0), ("f32", 12)])
def test_encode_leaves_the_sentinels_wherever_the_output_starts(fmt, lead, plane_files):
    """The last file is 1025 frames x 6 channels; with the others' odd frame counts x 3 channels the s24 data ends off a dword,
    and `lead` moves every file start across the four byte positions of a dword."""
    f = plane_files[fmt]
    got, counts, _ = _raw_encode(f, fmt, lead)
    assert got.tobytes() == f["data"] and counts.tolist() == f["clipped"]


def test_s24_odd_frames_of_three_channels_end_off_a_dword():
    p = (np.linspace(-1.2, 1.2, 3 * 7, dtype=np.float32)).reshape(3, 7)
    f = dict(planes=[p], frames=[7])
    want, n = R.encode(p, "s24", 7)
    assert len(want) == 63 and len(want) % 4 == 3
    for lead in range(4):
        got, counts, _ = _raw_encode(f, "s24", lead)
        assert got.tobytes() == want and counts.tolist() == [n]


@pytest.mark.parametrize("fmt", ["s24", "s16"])
@pytest.mark.parametrize("col,value", [(0, 1 << 40), (0, -1), (1, 1 << 40), (1, -1), (2, 0), (2, 65), (3, 1 << 40), (3, -2), (4, 1 << 40),
                                       (4, -8)],
                         ids=["first-far", "first<0", "available-huge", "available<0", "channels=0", "channels=65", "frames-huge",
                              "frames<0", "out-far", "out<0"])
def test_encode_skips_a_device_row_outside_the_totals(fmt, col, value, plane_files):
    f, victim = plane_files[fmt], 25                            # 257 frames x 3 channels
    got, counts, off = _raw_encode(f, fmt, 1 if fmt == "s24" else 0, _corrupt(victim, col, value))
    end = list(off[1:]) + [len(got)]
    for j in range(len(f["planes"])):
        mine, want = got[off[j]:end[j]].tobytes(), f["data"][off[j]:end[j]]
        if j == victim:
            assert mine == bytes([SENTINEL]) * len(want) and counts[j] == 0, "a row outside the totals was followed"
        else:
            assert mine == want and counts[j] == f["clipped"][j], j


# ------------------------------------------------------------------------------------------------ past one pass of the grid
def test_a_file_longer_than_one_pass_of_the_grid():
    from sos_amd import audio_io
    rng = np.random.default_rng(47)
    n = 600000                                                  # x 2 channels = 1.2 M elements > 1024 x 256 x 4
    a = rng.integers(-32768, 32767, size=(n, 2), endpoint=True).astype(np.int16)
    y = audio_io.decode_planes_batch_device([a], ["s16"])[0]
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(R.decode(a, "s16")))
    p = rng.uniform(-1.1, 1.1, size=(2, n)).astype(np.float32)
    dev = torch.from_numpy(p).cuda()
    for fmt in ("s24", "s16"):
        data, _, clipped = audio_io.encode_batch_device([dev], fmt, frames=[n + 5])
        want, count = R.encode(p, fmt, n + 5)
        assert data.cpu().numpy().tobytes() == want and clipped.cpu().tolist() == [count] and count > 0
