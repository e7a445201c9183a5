"""wave_file.py on the host: the one chunk walker under wave_info (chunk heads only) and read_wave_info (heads, then the samples),
and the one table of sample formats with the views derived from it.  The two readers must agree on every file -- equal `info`
dicts, or WaveFormatError with equal text, and no other exception class -- and wave_info must never read the samples."""
import builtins
import struct

import numpy as np
import pytest

RATE = 8000


def _chunk(cid, body, size=None):
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\x00" if len(body) & 1 else b"")


def _riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _fmt(tag, ch, bits, extra=b"", size=None):
    align = ch * (bits // 8)
    return _chunk(b"fmt ", struct.pack("<HHIIHH", tag, ch, RATE, RATE * align, align, bits) + extra, size)


def _extensible(sub_tag, bits):
    """The 24 bytes after the 16 of a WAVE_FORMAT_EXTENSIBLE fmt chunk: cbSize, valid bits, channel mask, sub-format GUID."""
    return struct.pack("<HHI", 22, bits, 3) + struct.pack("<H", sub_tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"


DATA = bytes(range(48))                                     # whole frames of 1 and 2 channels of every width of the table

# name -> (the file's bytes, None if readable or the text after "<path>: " of the refusal)
DEFECTS = {
    "0 bits": (_riff(_fmt(1, 1, 0), _chunk(b"data", DATA)), "unsupported WAVE format tag 1 with 0 bits"),
    "4 bits": (_riff(_fmt(1, 1, 4), _chunk(b"data", DATA)), "unsupported WAVE format tag 1 with 4 bits"),
    "12 bits": (_riff(_fmt(1, 1, 12), _chunk(b"data", DATA)), "unsupported WAVE format tag 1 with 12 bits"),
    "cut inside fmt": (_riff(_fmt(1, 2, 16), _chunk(b"data", DATA))[:12 + 8 + 10], "short fmt chunk"),
    "cut inside the extension": (_riff(_fmt(0xFFFE, 2, 16, _extensible(1, 16)), _chunk(b"data", DATA))[:12 + 8 + 20],
                                 "missing fmt or data chunk"),
    "fmt of 14 bytes": (_riff(_chunk(b"fmt ", struct.pack("<HHIIH", 1, 1, RATE, RATE * 2, 2)), _chunk(b"data", DATA)), "short fmt chunk"),
    "data size beyond the file": (_riff(_fmt(1, 2, 16), _chunk(b"data", DATA[:12], size=1000)), None),
    "data cut in mid-frame": (_riff(_fmt(1, 2, 16), _chunk(b"data", DATA[:7], size=8))[:-1], None),
    "no data chunk": (_riff(_fmt(1, 2, 16), _chunk(b"LIST", b"abcd")), "missing fmt or data chunk"),
    "no fmt chunk": (_riff(_chunk(b"data", DATA)), "missing fmt or data chunk"),
    "0 channels": (_riff(_fmt(1, 0, 16), _chunk(b"data", DATA)), "no channels"),
    "dangling chunk head": (_riff(_fmt(1, 2, 16)) + b"da", "missing fmt or data chunk"),
    "odd LIST before data": (_riff(_fmt(1, 2, 16), _chunk(b"LIST", b"abcde"), _chunk(b"data", DATA)), None),
    "EXTENSIBLE, fmt of 16": (_riff(_fmt(0xFFFE, 2, 16), _chunk(b"data", DATA)), "unsupported WAVE format tag 65534 with 16 bits"),
    "EXTENSIBLE, fmt of 40, PCM 16": (_riff(_fmt(0xFFFE, 2, 16, _extensible(1, 16)), _chunk(b"data", DATA)), None),
    "not RIFF": (b"RIFX" + _riff(_fmt(1, 2, 16), _chunk(b"data", DATA))[4:], "not a RIFF/WAVE file"),
    "11 bytes": (b"RIFF\x04\x00\x00\x00WAV", "not a RIFF/WAVE file"),
}
READABLE_INFO = {
    "data size beyond the file": dict(tag=1, bits=16, channels=2, rate=RATE, frames=3),
    "data cut in mid-frame": dict(tag=1, bits=16, channels=2, rate=RATE, frames=1),
    "odd LIST before data": dict(tag=1, bits=16, channels=2, rate=RATE, frames=12),
    "EXTENSIBLE, fmt of 40, PCM 16": dict(tag=1, bits=16, channels=2, rate=RATE, frames=12),
}


def _table_files():
    """One file of every format of the table, mono and stereo: name -> (bytes, expected info)."""
    from sos_amd import wave_file
    files = {}
    for f in wave_file.FORMATS:
        for ch in (1, 2):
            blob = wave_file.wave_container(DATA, f.tag, ch, RATE, f.bits)
            files["%s x %d" % (f.name, ch)] = (blob, dict(tag=f.tag, bits=f.bits, channels=ch, rate=RATE, frames=len(DATA) // (f.width * ch)))
    return files


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, bytes, expected info or None, expected refusal or None)"""
    root = tmp_path_factory.mktemp("waves")
    every = {name: (blob, info, None) for name, (blob, info) in _table_files().items()}
    every.update({name: (blob, READABLE_INFO.get(name), refusal) for name, (blob, refusal) in DEFECTS.items()})
    assert set(READABLE_INFO) == {name for name, (_, refusal) in DEFECTS.items() if refusal is None}
    out = {}
    for k, (name, (blob, info, refusal)) in enumerate(every.items()):
        path = str(root / ("%02d.wav" % k))
        with open(path, "wb") as fp:
            fp.write(blob)
        out[name] = (path, blob, info, refusal)
    return out


def _outcome(fn):
    """What a reader answers: its result, or the text of its WaveFormatError; any other exception class escapes and fails the test."""
    from sos_amd import wave_file
    try:
        return "info", fn()
    except wave_file.WaveFormatError as e:
        return "refused", str(e)


def test_both_readers_agree_on_every_file(files):
    from sos_amd import wave_file
    assert len(files) == 2 * len(wave_file.FORMATS) + len(DEFECTS)
    for name, (path, _, info, refusal) in files.items():
        head = _outcome(lambda: wave_file.wave_info(path))
        whole = _outcome(lambda: wave_file.read_wave_info(path)[3])
        assert head == whole, name
        assert head == (("info", info) if refusal is None else ("refused", "%s: %s" % (path, refusal))), name


def test_the_samples_are_the_bytes_of_the_data_chunk(files):
    """Every readable file: (frames, channels) of the table's kind; the views that copy nothing hold the data's bytes, 24 bits sit in
    the top three bytes of an int32 and float64 is narrowed to float32."""
    from sos_amd import wave_file
    for name, (path, blob, info, refusal) in files.items():
        if refusal is not None:
            continue
        arr, kind, rate, got = wave_file.read_wave_info(path)
        f = wave_file.SOURCES[info["tag"], info["bits"]]
        at = blob.index(b"data") + 8
        data = blob[at:at + info["frames"] * info["channels"] * f.width]
        assert (kind, rate, got) == (f.kind, RATE, info) and arr.shape == (info["frames"], info["channels"]), name
        assert wave_file.read_wave(path)[1:] == (kind, rate) and np.array_equal(wave_file.read_wave(path)[0], arr, equal_nan=True)
        if f.name == "s24":
            assert arr.dtype == np.dtype("<i4") and arr.astype("<i4").tobytes() == b"".join(b"\x00" + data[i:i + 3] for i in range(0, len(data), 3))
        elif f.name == "f64":
            assert arr.dtype == np.float32 and np.array_equal(arr.reshape(-1), np.frombuffer(data, "<f8").astype(np.float32), equal_nan=True)
        else:
            assert arr.tobytes() == data and arr.flags.writeable, name


class _Counting:
    """An open file that counts the bytes it hands out."""

    def __init__(self, fp, count):
        self.fp, self.count = fp, count

    def read(self, n=-1):
        got = self.fp.read(n)
        self.count[0] += len(got)
        return got

    def readinto(self, buf):
        n = self.fp.readinto(buf)
        self.count[0] += n
        return n

    def __getattr__(self, name):
        return getattr(self.fp, name)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.fp.close()


def test_wave_info_reads_the_header_only(files, tmp_path, monkeypatch):
    """Fewer bytes than the header (everything before the samples) plus 64, whatever the data size; read_wave_info, through the same
    wrapper, reads the header and the samples (so the wrapper does count)."""
    from sos_amd import wave_file
    count = [0]
    monkeypatch.setattr(wave_file, "open", lambda path, mode: _Counting(builtins.open(path, mode), count), raising=False)
    big = str(tmp_path / "big.wav")
    blob = wave_file.wave_container(bytes(1 << 20), 3, 2, 48000, 32)
    with builtins.open(big, "wb") as fp:
        fp.write(blob)
    cases = [(big, blob)] + [(path, b) for path, b, _, refusal in files.values() if refusal is None]
    assert len(cases) == 1 + 2 * len(wave_file.FORMATS) + len(READABLE_INFO)
    for path, b in cases:
        header = b.index(b"data") + 8
        count[0] = 0
        info = wave_file.wave_info(path)
        assert 12 + 8 + 16 <= count[0] < header + 64, (path, count[0], header)
        count[0] = 0
        wave_file.read_wave_info(path)
        width = wave_file.SOURCES[info["tag"], info["bits"]].width
        assert count[0] >= header + info["frames"] * info["channels"] * width - 64, (path, count[0])


# ------------------------------------------------------------------------------------------------------ the format table
# the literals of the commit before the table
ENCODINGS = {"s16": (0, 2, 1, 16), "s32": (1, 4, 1, 32), "f32": (2, 4, 3, 32), "u8": (3, 1, 1, 8), "s24": (4, 3, 1, 24)}
G711 = {"alaw": (6, 1, 6, 8), "ulaw": (7, 1, 7, 8)}
SOURCE_FORMAT = {(1, 8): "u8", (1, 16): "s16", (1, 24): "s24", (1, 32): "s32", (3, 32): "f32", (3, 64): "f32", (6, 8): "alaw", (7, 8): "ulaw"}
PCM_CODES = {"s16": 0, "s32": 1, "f32": 2, "u8": 3}          # SOS_PCM_* of include/sos_hip.h


def test_the_derived_views_are_the_literals_they_replace():
    from sos_amd import audio_io, recordings, wave_file
    assert wave_file.ENCODINGS == ENCODINGS and wave_file.G711 == G711
    assert recordings.SAMPLE_FORMATS == {**ENCODINGS, **G711} and recordings._SOURCE_FORMAT == SOURCE_FORMAT
    assert wave_file._G711_KIND == {(6, 8): "alaw", (7, 8): "ulaw"}
    assert set(wave_file.SOURCES) == set(SOURCE_FORMAT)
    assert wave_file.DECODE == {**{k: ("pcm", c) for k, c in PCM_CODES.items()}, "alaw": ("g711", 6), "ulaw": ("g711", 7)}
    assert audio_io.ENCODINGS is wave_file.ENCODINGS and audio_io.G711 is wave_file.G711
    names = [f.name for f in wave_file.FORMATS]
    assert len(set(names)) == len(names) == len(wave_file.SOURCES)
    for f in wave_file.FORMATS:
        assert f.width * 8 == f.bits and f.kind in wave_file.DECODE and wave_file.DECODE[f.kind] == (f.family, f.decode)


def test_every_written_format_reads_back_as_itself(tmp_path):
    from sos_amd import recordings, wave_file
    for name, (_, width, tag, bits) in recordings.SAMPLE_FORMATS.items():
        for ch in (1, 2):
            path = str(tmp_path / ("%s_%d.wav" % (name, ch)))
            with open(path, "wb") as fp:
                fp.write(wave_file.wave_container(DATA, tag, ch, RATE, bits))
            info = wave_file.wave_info(path)
            assert info == dict(tag=tag, bits=bits, channels=ch, rate=RATE, frames=len(DATA) // (width * ch)), name
            assert recordings._SOURCE_FORMAT[info["tag"], info["bits"]] == name


def test_wave_container_refusals_are_unchanged():
    from sos_amd import wave_file
    for tag, ch, bits in ((2, 1, 16), (6, 1, 16), (7, 2, 32), (1, 1, 12), (1, 1, 0), (3, 0, 32)):
        with pytest.raises(ValueError, match=r"wave_container: tag 1 \(PCM\), 3 \(float\) or 6 / 7"):
            wave_file.wave_container(b"", tag, ch, RATE, bits)
    with pytest.raises(ValueError, match="47 bytes are no whole number of 4-byte frames"):
        wave_file.wave_container(DATA[:47], 1, 2, RATE, 16)
    assert wave_file.wave_container(DATA, 1, 2, RATE, 64)[:4] == b"RIFF"          # any whole number of bytes under a linear tag


def test_file_groups_count_a_refused_file_as_empty(files):
    from sos_amd import wave_file
    order = ["s16 x 1", "0 bits", "f64 x 2", "cut inside fmt", "alaw x 2"]
    frames = [48 // 2, 0, 48 // 16, 0, 48 // 2]
    assert wave_file.file_groups([files[n][0] for n in order] + ["/nonexistent/x.wav"], 4 * (frames[0] + frames[2])) == [[0, 1, 2, 3], [4, 5]]
