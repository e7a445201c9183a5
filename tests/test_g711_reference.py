"""tests/g711_reference.py against CPython's audioop (its copy of the Sun / ITU g711.c) over the WHOLE domain -- 256 codes in,
65 536 s16 values out -- and the host side of G.711 in the package: the WAVE container (tags 6 / 7) written and parsed, the
host refusals of sos_g711_planes_batch_f32 / sos_g711_encode_batch / sos_g711_to_mono_f32 (the device pointers are dummies that
are never dereferenced) and the argument errors of the Python functions.  No GPU."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import g711_reference as G
import pcm_reference as R
from test_pcm_host_cpu import P, _edit, _host, _refused, encode_table, planes_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAWS = ("alaw", "ulaw")
CODES = np.arange(256, dtype=np.uint8)
S16 = np.arange(-32768, 32768, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("law", LAWS)
def test_expand_is_audioop_on_every_code(law):
    audioop = pytest.importorskip("audioop")
    raw = (audioop.alaw2lin if law == "alaw" else audioop.ulaw2lin)(CODES.tobytes(), 2)
    assert np.array_equal(G.expand(CODES, law), np.frombuffer(raw, dtype="<i2").astype(np.int64))


@pytest.mark.parametrize("law", LAWS)
def test_compress_is_audioop_on_every_s16_value(law):
    audioop = pytest.importorskip("audioop")
    raw = (audioop.lin2alaw if law == "alaw" else audioop.lin2ulaw)(S16.astype("<i2").tobytes(), 2)
    got = G.compress(S16, law)
    differ = np.flatnonzero(got != np.frombuffer(raw, dtype=np.uint8))
    assert differ.size == 0, (law, S16[differ[:8]], got[differ[:8]])


@pytest.mark.parametrize("law", LAWS)
def test_ranges_levels_round_trip_and_silence(law):
    lin = G.expand(CODES, law)
    assert lin.max() == G.PEAK[law] == -lin.min() and G.PEAK == dict(alaw=32256, ulaw=32124)
    assert len(set(lin.tolist())) == (256 if law == "alaw" else 255)             # mu-law has two zeros
    back = G.compress(lin, law)
    want = CODES.copy()
    if law == "ulaw":
        assert lin[0x7F] == 0 == lin[0xFF]
        want[0x7F] = 0xFF                                                         # negative zero comes back as zero
    assert np.array_equal(back, want)
    assert G.compress(np.zeros(1, np.int64), law)[0] == G.SILENCE[law] == dict(alaw=0xD5, ulaw=0xFF)[law]
    assert G.expand(np.zeros(1, np.uint8), law)[0] == dict(alaw=-5504, ulaw=-32124)[law]     # byte 0 is far from silence
    planes = G.decode(CODES.reshape(-1, 1), law)                                  # value = level / 32768, exact in f32
    assert planes.dtype == np.float32 and np.array_equal(planes[0].astype(np.float64) * 32768.0, lin.astype(np.float64))
    data, clipped = G.encode(planes, law, frames=300)
    assert clipped == 0 and data[:256] == want.tobytes() and data[256:] == bytes([G.SILENCE[law]]) * 44


def test_encode_counts_what_s16_counts():
    x = np.concatenate([R.edge_values("s16"), np.linspace(-1.5, 1.5, 97, dtype=np.float32)]).reshape(1, -1)
    for law in LAWS:
        data, clipped = G.encode(x, law)
        q, want = R.quantise(x.T, "s16")
        assert clipped == want > 0 and data == G.compress(q, law).tobytes()


# ------------------------------------------------------------------------------------------------ containers
def _codes(frames, channels, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(frames, channels), dtype=np.uint8)


def _extensible(blob, law, channels, rate):
    """The same data under a WAVE_FORMAT_EXTENSIBLE fmt chunk (40 bytes: cbSize 22, valid bits, channel mask, sub-format GUID
    whose first word is the tag), with an odd LIST chunk and its pad byte between fmt and data."""
    data = blob[blob.index(b"data") + 8:]
    guid = struct.pack("<H", G.TAG[law]) + bytes.fromhex("000000001000800000AA00389B71")
    fmt = struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * channels, channels, 8) + struct.pack("<HHI", 22, 8, 0) + guid
    assert len(fmt) == 40
    chunks = b"fmt " + struct.pack("<I", 40) + fmt + b"LIST" + struct.pack("<I", 5) + b"INFOx" + b"\0"
    chunks += b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("law", LAWS)
def test_containers_are_written_and_parsed(law, channels, tmp_path):
    from sos_amd import audio_io
    assert audio_io.G711 == {"alaw": (6, 1, 6, 8), "ulaw": (7, 1, 7, 8)}
    codes, rate, frames = _codes(37, channels, 3 + channels), 8000, 37            # 37 x 1: an odd data chunk, no pad byte
    blob = G.container(codes.tobytes(), law, channels, rate)
    assert audio_io.wave_container(codes.tobytes(), G.TAG[law], channels, rate, 8) == blob
    assert len(blob) == 12 + 8 + 18 + 8 + 4 + 8 + frames * channels and blob[20:22] == struct.pack("<H", G.TAG[law])
    for name, content in (("plain.wav", blob), ("ext.wav", _extensible(blob, law, channels, rate))):
        path = tmp_path / name
        path.write_bytes(content)
        arr, kind, got_rate, info = audio_io.read_wave_info(str(path))
        assert kind == law and got_rate == rate and arr.dtype == np.uint8 and np.array_equal(arr, codes)
        assert audio_io.read_wave(str(path))[1:] == (law, rate)
        assert info == dict(tag=G.TAG[law], bits=8, channels=channels, rate=rate, frames=frames) == audio_io.wave_info(str(path))
    with pytest.raises(ValueError):
        audio_io.wave_container(codes.tobytes(), G.TAG[law], channels, rate, 16)  # G.711 is 8 bits
    path.write_bytes(blob[:34] + struct.pack("<H", 16) + blob[36:])               # the fmt chunk's bits field
    for parse in (audio_io.read_wave_info, audio_io.wave_info):
        with pytest.raises(audio_io.WaveFormatError, match="unsupported WAVE format tag %d with 16 bits" % G.TAG[law]):
            parse(str(path))


def test_file_groups_count_four_bytes_per_frame(tmp_path):
    from sos_amd import audio_io
    paths = []
    for k, (law, ch, frames) in enumerate((("ulaw", 1, 1000), ("alaw", 2, 500), ("ulaw", 1, 250))):
        paths.append(str(tmp_path / ("%d.wav" % k)))
        with open(paths[-1], "wb") as fp:
            fp.write(G.container(_codes(frames, ch, k).tobytes(), law, ch, 8000))
    assert audio_io.file_groups(paths, 6000) == [[0, 1], [2]]                    # 4000 + 2000 bytes of mono f32, then 1000
    assert audio_io.file_groups(paths, 4000) == [[0], [1, 2]]


# ------------------------------------------------------------------------------------------------ the C ABI, host side
def _planes(tab=None, nfiles=3, law=7, null=None):
    from sos_amd import _lib as L
    tab = planes_table() if tab is None else tab
    a = dict(codes=P, table=P, table_host=_host(tab), out=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_g711_planes_batch_f32(a["codes"], law, a["table"], a["table_host"], nfiles, a["out"], None)
    return rc, h.sos_last_error().decode(), "sos_g711_planes_batch_f32:"


def _encode(tab=None, nfiles=3, law=6, null=None):
    from sos_amd import _lib as L
    tab = encode_table() if tab is None else tab
    a = dict(planes=P, table=P, table_host=_host(tab), out=P, clipped=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_g711_encode_batch(a["planes"], a["table"], a["table_host"], nfiles, law, a["out"], a["clipped"], None)
    return rc, h.sos_last_error().decode(), "sos_g711_encode_batch:"


def _mono(law=7, channels=2, frames=10, null=None):
    from sos_amd import _lib as L
    a = dict(codes=P, out=P)
    if null:
        a[null] = None
    h = L.lib()
    rc = h.sos_g711_to_mono_f32(a["codes"], law, channels, frames, a["out"], None)
    return rc, h.sos_last_error().decode(), "sos_g711_to_mono_f32:"


def test_header_declares_and_library_exports_the_three_symbols():
    from sos_amd import _lib as L
    from sos_amd import audio_io
    hdr = open(os.path.join(ROOT, "include", "sos_hip.h")).read()
    h = L.lib()
    for name, nargs in (("sos_g711_planes_batch_f32", 7), ("sos_g711_encode_batch", 8), ("sos_g711_to_mono_f32", 6)):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(h, name) and len(L.SIGNATURES[name]) == nargs
    assert re.search(r"enum\s*\{\s*SOS_G711_ALAW = 6, SOS_G711_ULAW = 7\s*\}", hdr), "the laws are the WAVE format tags"
    assert h.sos_abi_version() == L.EXPECTED_ABI == 10          # added symbols break no caller
    assert audio_io.ENCODINGS == {"s16": (0, 2, 1, 16), "s32": (1, 4, 1, 32), "f32": (2, 4, 3, 32), "u8": (3, 1, 1, 8), "s24": (4, 3, 1, 24)}


@pytest.mark.parametrize("call,names", [(_planes, ["codes", "table", "table_host", "out"]),
                                        (_encode, ["planes", "table", "table_host", "out", "clipped"])], ids=["decode", "encode"])
def test_batch_entry_points_refuse_null_pointers_counts_and_laws(call, names):
    for name in names:
        _refused(call(null=name), "null pointer")
    _refused(call(nfiles=0), "1 .. 65535 files, got 0")
    _refused(call(nfiles=65536), "1 .. 65535 files, got 65536")
    for law in (0, 5, 8):                                                        # a PCM code, none at all, one past mu-law
        _refused(call(law=law), "unknown law %d" % law)


def test_mono_entry_point_refuses_null_pointers_shapes_and_laws():
    for name in ("codes", "out"):
        _refused(_mono(null=name), "bad args")
    _refused(_mono(channels=0), "channels=0")
    _refused(_mono(channels=65), "channels=65")
    _refused(_mono(frames=0), "n_frames=0")
    for law in (0, 5, 8):
        _refused(_mono(law=law), "unknown law %d" % law)


def test_one_bad_table_row_is_named_by_file():
    _refused(_planes(tab=_edit(planes_table, 1, 2, 0)), "file 1", "channels outside 1 .. 64")
    _refused(_planes(tab=_edit(planes_table, 2, 0, 516)), "file 2 (pcm element 516, 1025 frames, 3 channels, output 515)",
             "outside the totals", "3590 elements")
    _refused(_planes(tab=_edit(planes_table, 0, 1, -1)), "file 0", "-1 frames", "negative or too large")
    _refused(_encode(tab=_edit(encode_table, 0, 2, 65)), "file 0", "65 channels")
    _refused(_encode(tab=_edit(encode_table, 2, 4, 402)), "file 2", "output element 402", "outside the totals", "3701 output elements")
    _refused(_encode(tab=_edit(encode_table, 2, 1, -5)), "file 2", "-5 available", "negative or too large")


# ------------------------------------------------------------------------------------------------ Python arguments
def test_argument_errors_are_raised_without_a_gpu(tmp_path):
    import torch
    from sos_amd import audio_io, recordings
    with pytest.raises(ValueError, match="unknown law 'mulaw'"):
        audio_io.g711_decode_device(np.zeros(4, np.uint8), "mulaw")
    with pytest.raises(ValueError, match="unknown law 'u8'"):
        audio_io.g711_encode_device(torch.zeros(4), "u8")
    with pytest.raises(ValueError, match="1-D uint8"):
        audio_io.g711_decode_device(np.zeros((4, 1), np.uint8), "ulaw")
    with pytest.raises(ValueError, match="1-D uint8"):
        audio_io.g711_decode_device(np.zeros(4, np.int16), "alaw")
    with pytest.raises(ValueError, match="1-D float32"):
        audio_io.g711_encode_device(torch.zeros(1, 4), "alaw")
    with pytest.raises(ValueError, match="file 0 must be"):
        audio_io.encode_batch_device([torch.zeros(4)], "ulaw")
    with pytest.raises(ValueError, match="file 1 must be"):
        audio_io.decode_planes_batch_device([np.zeros((4, 1), np.uint8), np.zeros(4, np.uint8)], ["ulaw", "alaw"])
    with pytest.raises(RuntimeError, match="MI355X"):                            # no CPU fallback
        audio_io.g711_encode_device(torch.zeros(4), "ulaw")
    with pytest.raises(RuntimeError, match="MI355X"):
        audio_io.pcm_to_mono_device(torch.zeros((4, 2), dtype=torch.uint8), "alaw")
    assert recordings._SOURCE_FORMAT[6, 8] == "alaw" and recordings._SOURCE_FORMAT[7, 8] == "ulaw"
    with pytest.raises(ValueError, match="unsupported sample_format 'mulaw'"):
        recordings.denoise_recordings(None, None, [], str(tmp_path), sample_format="mulaw")
    short = tmp_path / "short.wav"                                               # accepted as a format, refused for its length
    short.write_bytes(G.container(bytes([0xFF]) * 800, "ulaw", 1, 8000))
    with pytest.raises(ValueError, match="recordings need at least"):
        recordings.denoise_recordings(None, None, [str(short)], str(tmp_path / "out"), sample_format="alaw")
