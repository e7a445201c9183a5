"""audio_io.file_groups: the bytes it counts per file are the mono f32 samples audio_io.read_wave decodes, in every format the
loader takes; what cannot be read counts 0; the groups are ragged.byte_groups of those sizes.  No GPU."""
import struct

import numpy as np

# (format tag, stored bits, channels, frames): every sample format of read_wave, mono and stereo among them
FORMATS = [(1, 8, 1, 31), (1, 16, 2, 40), (1, 24, 1, 17), (1, 24, 2, 23), (1, 32, 1, 29), (3, 32, 2, 35), (3, 64, 1, 19)]


def _files(tmp_path):
    from sos_amd import audio_io
    rng = np.random.default_rng(3)
    paths = []
    for tag, bits, ch, frames in FORMATS:
        data = rng.integers(0, 256, size=frames * ch * (bits // 8), dtype=np.uint8)
        if tag == 3:                                                             # finite floats
            data = rng.uniform(-1, 1, size=frames * ch).astype("<f4" if bits == 32 else "<f8").view(np.uint8)
        paths.append(str(tmp_path / ("t%d_b%d_c%d.wav" % (tag, bits, ch))))
        with open(paths[-1], "wb") as fp:
            fp.write(audio_io.wave_container(data.tobytes(), tag, ch, 16000, bits))
    # an extra chunk of odd size (and its pad byte) between fmt and data
    blob = audio_io.wave_container(rng.integers(-2000, 2000, size=2 * 27, dtype=np.int16).tobytes(), 1, 2, 44100, 16)
    at = blob.index(b"data")
    blob = blob[:at] + b"LIST" + struct.pack("<I", 5) + b"INFOx" + b"\0" + blob[at:]
    blob = blob[:4] + struct.pack("<I", len(blob) - 8) + blob[8:]
    paths.append(str(tmp_path / "extra_chunk.wav"))
    with open(paths[-1], "wb") as fp:
        fp.write(blob)
    return paths


def _counts(path, size):
    """Whether file_groups counts `size` bytes for the file: the file twice is one group at a budget of 2 size bytes (it counts
    no more) and two groups at one byte less (it counts no less)."""
    from sos_amd import audio_io
    return audio_io.file_groups([path, path], 2 * size) == [[0, 1]] and \
        (size == 0 or audio_io.file_groups([path, path], 2 * size - 1) == [[0], [1]])


def test_file_groups_counts_what_the_loader_decodes(tmp_path):
    from sos_amd import audio_io, ragged
    paths = _files(tmp_path)
    want = [4 * len(audio_io.read_wave(p)[0]) for p in paths]
    assert want == [4 * f[3] for f in FORMATS] + [4 * 27]
    for p, size in zip(paths, want):
        assert _counts(p, size), (p, size)
    bad = str(tmp_path / "not_riff.wav")
    with open(bad, "wb") as fp:
        fp.write(b"RIFX" + b"\0" * 60)
    missing = str(tmp_path / "missing.wav")
    assert _counts(bad, 0) and _counts(missing, 0)
    every, sizes = paths + [bad, missing], want + [0, 0]
    for budget in (0, 100, 160, 256, 1 << 30):
        groups = audio_io.file_groups(every, budget)
        assert groups == ragged.byte_groups(sizes, budget)
        assert [i for g in groups for i in g] == list(range(len(every)))
    assert len(audio_io.file_groups(every, 160)) > 2 and audio_io.file_groups(every, 1 << 30) == [list(range(len(every)))]
