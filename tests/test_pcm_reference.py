"""tests/pcm_reference.py against the rule as include/sos_hip.h states it, against itself (round trips) and against independent
WAVE parsers; audio_io.wave_container against the reference container and wave_bytes.  No GPU."""
import io
import wave

import numpy as np
import pytest

import pcm_reference as R

INT_FORMATS = ["s16", "s24", "s32", "u8"]
FORMATS = INT_FORMATS + ["f32"]


def _q(x, fmt):
    q, n = R.quantise(np.asarray([x], dtype=np.float32), fmt)
    return int(q[0]), n


@pytest.mark.parametrize("fmt", INT_FORMATS)
def test_ties_go_to_even_and_the_ends_saturate(fmt):
    S = R.scale(fmt)
    assert _q(0.5 / S, fmt) == (0, 0) and _q(1.5 / S, fmt) == (2, 0) and _q(2.5 / S, fmt) == (2, 0) and _q(-0.5 / S, fmt) == (0, 0)
    assert _q(-1.0, fmt) == (-int(S), 0)                       # -1.0 is the format's lowest value: not counted
    assert _q(1.0, fmt) == (int(S) - 1, 1)                     # +1.0 is one past its highest: saturated, counted
    assert _q(np.nan, fmt) == (0, 1)
    assert _q(np.inf, fmt) == (int(S) - 1, 1) and _q(-np.inf, fmt) == (-int(S), 1)
    assert _q(-0.0, fmt) == (0, 0) and _q(1e-45, fmt) == (0, 0)


def test_u8_is_offset_binary_and_s24_is_three_little_endian_bytes():
    p = np.asarray([[-1.0, 0.0, 1.0, 0.5]], dtype=np.float32)
    assert R.encode(p, "u8") == (bytes([0, 128, 255, 192]), 1)
    data, n = R.encode(np.asarray([[-1.0, 1.0 / 8388608.0, 1.0, -1.0 / 8388608.0]], dtype=np.float32), "s24")
    assert data == bytes([0, 0, 0x80, 1, 0, 0, 0xFF, 0xFF, 0x7F, 0xFF, 0xFF, 0xFF]) and n == 1
    assert R.encode(p, "f32") == (p.tobytes(), 0)


def test_frames_crop_and_zero_fill():
    p = np.asarray([[0.25, 0.5, 0.75], [-0.25, -0.5, -0.75]], dtype=np.float32)
    assert R.unpack(R.encode(p, "s16", 2)[0], "s16", 2).tolist() == [[8192, -8192], [16384, -16384]]
    assert R.unpack(R.encode(p, "s16", 5)[0], "s16", 2).tolist() == [[8192, -8192], [16384, -16384], [24576, -24576], [0, 0], [0, 0]]
    assert R.encode(p, "u8", 4)[0][-2:] == bytes([128, 128])     # u8 silence is 128
    assert R.encode(p, "s24", 0) == (b"", 0)


def _all_values(fmt):
    if fmt == "s16":
        return np.arange(-32768, 32768, dtype=np.int64)
    if fmt == "u8":
        return np.arange(0, 256, dtype=np.int64)
    if fmt == "s24":
        return np.unique(np.concatenate([np.arange(-2 ** 23, 2 ** 23, 977), [-2 ** 23, -2 ** 23 + 1, -1, 0, 1, 2 ** 23 - 2, 2 ** 23 - 1]]))
    if fmt == "s32":
        return np.unique(np.concatenate([np.arange(-2 ** 31, 2 ** 31, 65521 * 7), [-2 ** 31, -2 ** 31 + 1, -129, -128, -1, 0, 1, 127, 128,
                                                                              2 ** 31 - 129, 2 ** 31 - 128, 2 ** 31 - 2, 2 ** 31 - 1]]))
    return np.concatenate([R.edge_values("f32")[np.isfinite(R.edge_values("f32"))], np.linspace(-1.5, 1.5, 1001)]).astype(np.float32)


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_encode_decode_is_decode(fmt):
    v = _all_values(fmt).reshape(-1, 1)
    planes = R.decode(v, fmt)
    again = R.decode(R.unpack(R.encode(planes, fmt)[0], fmt, 1), fmt)
    assert again.dtype == planes.dtype == np.float32 and np.array_equal(again.view(np.uint32), planes.view(np.uint32))


@pytest.mark.parametrize("fmt", ["s16", "u8", "s24"])
def test_encode_decode_is_the_identity_on_stored_values(fmt):
    """All values of s16 and u8, a stride through s24 with both ends: what fits a float32 exactly comes back, none counted."""
    v = _all_values(fmt).reshape(-1, 1)
    data, clipped = R.encode(R.decode(v, fmt), fmt)
    assert clipped == 0 and np.array_equal(R.unpack(data, fmt, 1), v)


def _signal(frames, channels, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, size=(channels, frames)) * 0.99).astype(np.float32)


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
@pytest.mark.parametrize("fmt", FORMATS)
def test_containers_parse_with_read_wave_and_independent_readers(fmt, channels, tmp_path):
    from sos_amd import audio_io
    planes, rate = _signal(37, channels, channels), 44100
    data, _ = R.encode(planes, fmt)
    blob = R.container(data, fmt, channels, rate)
    tag, bits = R.TAG_BITS[fmt]
    assert audio_io.wave_container(data, tag, channels, rate, bits) == blob
    path = tmp_path / "x.wav"
    path.write_bytes(blob)
    want = R.decode(R.unpack(data, fmt, channels), fmt)                       # what the file holds, as planes
    arr, kind, got_rate, info = audio_io.read_wave_info(str(path))
    assert audio_io.read_wave(str(path))[1:] == (kind, got_rate) and got_rate == rate
    assert info == dict(tag=tag, bits=bits, channels=channels, rate=rate, frames=37) == audio_io.wave_info(str(path))
    assert kind == ("s32" if fmt == "s24" else fmt) and arr.shape == (37, channels)
    carried = R.unpack(data, fmt, channels) * 256 if fmt == "s24" else R.unpack(data, fmt, channels)
    assert np.array_equal(arr.astype(carried.dtype), carried)
    assert np.array_equal(R.decode(arr, kind), want)                          # s24 carried as s32 decodes to the same planes
    if tag == 1:
        with wave.open(io.BytesIO(blob)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (channels, bits // 8, rate, 37)
            assert w.readframes(37) == data
    if fmt in ("s16", "f32"):
        try:
            from scipy.io import wavfile
        except ImportError:                                                   # a third reader where there is one
            return
        sr, y = wavfile.read(str(path))
        assert sr == rate and np.array_equal(y.reshape(37, channels), R.unpack(data, fmt, channels).astype(y.dtype))


def test_wave_container_is_wave_bytes_for_float_data():
    from sos_amd import audio_io
    y = _signal(129, 1, 5)[0]
    assert audio_io.wave_container(y.tobytes(), 3, 1, 14000, 32) == audio_io.wave_bytes(y, 14000) == R.container(y.tobytes(), "f32", 1, 14000)
    y2 = np.ascontiguousarray(_signal(129, 2, 6).T)
    assert audio_io.wave_container(y2.tobytes(), 3, 2, 48000, 32) == audio_io.wave_bytes(y2, 48000)
    s = (y * 32767).astype(np.int16)
    assert audio_io.wave_container(s.tobytes(), 1, 1, 8000, 16) == audio_io.wave_bytes(s, 8000)
    with pytest.raises(ValueError):
        audio_io.wave_container(b"\0" * 5, 1, 2, 8000, 16)


def test_read_wave_keeps_its_three_values_and_reports_stored_bits_beside_it(tmp_path):
    from sos_amd import audio_io
    path = tmp_path / "d.wav"
    y = _signal(20, 2, 9).T.astype(np.float64)
    path.write_bytes(audio_io.wave_bytes(np.ascontiguousarray(y), 16000))
    got = audio_io.read_wave(str(path))
    assert len(got) == 3 and got[1:] == ("f32", 16000) and got[0].dtype == np.float32
    assert audio_io.read_wave_info(str(path))[3] == dict(tag=3, bits=64, channels=2, rate=16000, frames=20)
    for bad in (b"RIFF\0\0\0\0WAVX", R.container(b"", "s16", 1, 8000).replace(b"data", b"dat_")):
        path.write_bytes(bad)
        with pytest.raises(audio_io.WaveFormatError):
            audio_io.wave_info(str(path))
