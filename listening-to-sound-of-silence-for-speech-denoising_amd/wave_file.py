"""The RIFF/WAVE container, on the host only (bytes -> header fields + one frombuffer view, no per-sample Python; nothing here
touches the GPU): the table of sample formats, one chunk walker under read_wave / read_wave_info / wave_info / file_groups, and
the writers wave_bytes / wave_container / write_wav.  Sample conversion is the kernels' (planes.py, csrc/pcm_io.hip)."""
import os
import struct
from collections import namedtuple

import numpy as np
import torch

from . import ragged


class WaveFormatError(ValueError):
    pass


def _view(dtype):
    return lambda data: np.frombuffer(data, dtype=dtype)


def _widen_s24(data):                                       # widen to the top three bytes of an int32
    b3 = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3)
    arr = np.zeros((b3.shape[0], 4), dtype=np.uint8)
    arr[:, 1:] = b3
    return arr.view("<i4").reshape(-1)


# Every sample format, once.  name; tag, bits: the WAVE format tag and the bits per sample as stored; width: bytes per stored
# element; view: the stored data bytes -> the 1-D array the reader hands on; kind: what that array holds for the decode kernels;
# family, decode: their entry points ('pcm': sos_pcm_*, 'g711': sos_g711_*) and code (SOS_PCM_* of include/sos_hip.h, or the
# G.711 tag); encode: SOS_ENC_* or the G.711 tag (None: not a format that is written); back: the name a source of (tag, bits) is
# written back as.  A float64 source is carried, and written, as f32 (the networks compute in f32 at best); 24 bits are carried
# as s32; G.711 (telephone audio) travels as its code bytes, which the kernels expand, and comes back as G.711 of its own law.
Format = namedtuple("Format", "name tag bits width view kind family decode encode back")
FORMATS = (
    Format("s16", 1, 16, 2, _view("<i2"), "s16", "pcm", 0, 0, "s16"),
    Format("s32", 1, 32, 4, _view("<i4"), "s32", "pcm", 1, 1, "s32"),
    Format("f32", 3, 32, 4, _view("<f4"), "f32", "pcm", 2, 2, "f32"),
    Format("u8", 1, 8, 1, _view(np.uint8), "u8", "pcm", 3, 3, "u8"),
    Format("s24", 1, 24, 3, _widen_s24, "s32", "pcm", 1, 4, "s24"),
    Format("f64", 3, 64, 8, lambda data: np.frombuffer(data, dtype="<f8").astype(np.float32), "f32", "pcm", 2, None, "f32"),
    Format("alaw", 6, 8, 1, _view(np.uint8), "alaw", "g711", 6, 6, "alaw"),
    Format("ulaw", 7, 8, 1, _view(np.uint8), "ulaw", "g711", 7, 7, "ulaw"),
)
SOURCES = {(f.tag, f.bits): f for f in FORMATS}             # what the readers accept
DECODE = {f.kind: (f.family, f.decode) for f in FORMATS if f.name == f.kind}      # the kinds a reader yields
# encode formats: name -> (SOS_ENC_* of include/sos_hip.h, bytes per element, WAVE format tag, stored bits)
ENCODINGS = {f.name: (f.encode, f.width, f.tag, f.bits) for f in FORMATS if f.family == "pcm" and f.encode is not None}
# G.711, one code byte per sample: name -> (SOS_G711_* of include/sos_hip.h = the WAVE format tag, bytes per element, tag, bits)
G711 = {f.name: (f.encode, f.width, f.tag, f.bits) for f in FORMATS if f.family == "g711"}
_G711_KIND = {(v[2], v[3]): k for k, v in G711.items()}
_LINEAR_TAGS = {f.tag for f in FORMATS if f.family == "pcm"}


def _walk(fp, path):
    """The chunks of an open WAVE file up to the head of `data`; only chunk heads and the body of `fmt ` are read.  -> (the
    Format of the source, channels, rate, where the data start, their bytes cut at the end of the file).  Every refusal of the
    readers is made here."""
    size_all = os.fstat(fp.fileno()).st_size
    head = fp.read(12)
    if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
        raise WaveFormatError("%s: not a RIFF/WAVE file" % path)
    fmt, span = None, None
    while True:
        ck = fp.read(8)
        if len(ck) < 8:
            break
        cid, size = ck[:4], struct.unpack("<I", ck[4:])[0]
        if cid == b"fmt ":
            body = fp.read(size + (size & 1))
            if size < 16 or len(body) < 16:
                raise WaveFormatError("%s: short fmt chunk" % path)
            tag, ch, rate, _, _, bits = struct.unpack_from("<HHIIHH", body, 0)
            if tag == 0xFFFE and size >= 26 and len(body) >= 26:    # WAVE_FORMAT_EXTENSIBLE: the sub-format GUID's first word
                tag = struct.unpack_from("<H", body, 24)[0]
            fmt = (tag, ch, rate, bits)
        elif cid == b"data":
            span = (fp.tell(), max(0, min(size, size_all - fp.tell())))
            break
        else:
            fp.seek(size + (size & 1), os.SEEK_CUR)
    if fmt is None or span is None:
        raise WaveFormatError("%s: missing fmt or data chunk" % path)
    tag, ch, rate, bits = fmt
    if ch < 1:
        raise WaveFormatError("%s: no channels" % path)
    if (tag, bits) not in SOURCES:
        raise WaveFormatError("%s: unsupported WAVE format tag %d with %d bits" % (path, tag, bits))
    return (SOURCES[tag, bits], ch, rate) + span


def read_wave(path):
    """Parse a RIFF/WAVE file -> (samples ndarray (n_frames, channels) in a kernel format, fmt, sample rate).
    PCM 8/16/24/32-bit, IEEE float 32/64, G.711 A-law / mu-law (tags 6 / 7 with 8 bits: the uint8 code bytes, fmt 'alaw' /
    'ulaw'), WAVE_FORMAT_EXTENSIBLE wrappers of those."""
    return read_wave_info(path)[:3]


def read_wave_info(path):
    """read_wave plus what the file itself stores: (samples, fmt, sample rate, info) with info = dict(tag, bits, channels, rate,
    frames) -- `bits` as stored, so 24 stays 24 although the samples are carried as s32, and 64 stays 64 although they are
    carried as f32."""
    with open(path, "rb") as fp:
        f, ch, rate, start, nbytes = _walk(fp, path)
        n = nbytes // (f.width * ch)
        buf = bytearray(n * f.width * ch)                   # writable backing store: the sample view goes to torch
        fp.seek(start)
        fp.readinto(buf)
    return f.view(buf).reshape(n, ch), f.kind, rate, dict(tag=f.tag, bits=f.bits, channels=ch, rate=rate, frames=n)


def wave_info(path):
    """read_wave_info's `info` from the chunk headers alone (the samples are not read), with the same refusals."""
    with open(path, "rb") as fp:
        f, ch, rate, _, nbytes = _walk(fp, path)
    return dict(tag=f.tag, bits=f.bits, channels=ch, rate=rate, frames=nbytes // (f.width * ch))


def file_groups(paths, max_bytes):
    """Consecutive files in groups of at most max_bytes of mono f32 samples at their native rates (a file larger than that is
    a group of its own), from the chunk headers alone: 4 bytes per frame wave_info counts, the frames the loader decodes.  A
    file that wave_info refuses counts 0 bytes: the loader reports what is wrong with it."""
    sizes = []
    for path in paths:
        try:
            sizes.append(4 * wave_info(path)["frames"])
        except (OSError, WaveFormatError):
            sizes.append(0)
    return ragged.byte_groups(sizes, max_bytes)


def wave_bytes(y, sr):
    """Bytes of the file `scipy.io.wavfile.write(path, sr, y)` produces (what librosa.output.write_wav calls):
    int16/int32/uint8 -> PCM; float32/float64 -> IEEE float with an 18-byte fmt chunk and a `fact` chunk."""
    y = np.asarray(y)
    if y.ndim == 1:
        ch = 1
    elif y.ndim == 2:
        ch = y.shape[1]
    else:
        raise ValueError("wave data must be (n,) or (n, channels)")
    kind = y.dtype.kind
    if not (kind in "iu" and y.dtype.itemsize in (1, 2, 4, 8) or kind == "f" and y.dtype.itemsize in (4, 8)):
        raise ValueError("Unsupported data type '%s'" % y.dtype)
    if kind == "u" and y.dtype.itemsize != 1 or kind == "i" and y.dtype.itemsize == 1:
        raise ValueError("Unsupported data type '%s'" % y.dtype)
    tag = 3 if kind == "f" else 1
    bits = y.dtype.itemsize * 8
    data = np.ascontiguousarray(y).astype(y.dtype.newbyteorder("<"), copy=False).tobytes()
    return _riff(data, tag, ch, sr, bits, y.shape[0])


def _riff(data, tag, ch, sr, bits, frames):
    """The chunks around `data`: a 16-byte fmt chunk for PCM; an 18-byte one and a `fact` chunk with the frame count otherwise."""
    align = ch * (bits // 8)
    fmt = struct.pack("<HHIIHH", tag, ch, int(sr), int(sr) * align, align, bits)
    if tag != 1:
        fmt += b"\x00\x00"
    head = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if tag != 1:
        head += b"fact" + struct.pack("<II", 4, frames)
    if len(head) + len(data) + 12 > 0xFFFFFFFF:
        raise ValueError("Data exceeds wave file size limit")
    body = b"WAVE" + head + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def wave_container(data_bytes, tag, channels, rate, bits):
    """The RIFF/WAVE file around already-encoded interleaved data (encode_batch_device's bytes): tag 1 (PCM) with a 16-byte
    fmt chunk, tag 3 (IEEE float) with an 18-byte fmt chunk and a `fact` chunk, the chunks of wave_bytes -- for mono or
    interleaved f32 data, wave_container(y.tobytes(), 3, channels, sr, 32) == wave_bytes(y, sr).  Tags 6 / 7 (G.711 A-law /
    mu-law, 8 bits) get the chunks of every non-PCM format, the 18-byte fmt chunk and `fact`; like u8 data, an odd number of
    code bytes is followed by no pad byte."""
    data = bytes(data_bytes)
    if tag not in _LINEAR_TAGS and (tag, bits) not in _G711_KIND or bits % 8 or bits < 8 or channels < 1:
        raise ValueError("wave_container: tag 1 (PCM), 3 (float) or 6 / 7 (G.711 A-law / mu-law, 8 bits), whole bytes per sample, "
                         "at least one channel")
    align = channels * (bits // 8)
    if len(data) % align:
        raise ValueError("wave_container: %d bytes are no whole number of %d-byte frames" % (len(data), align))
    return _riff(data, tag, channels, rate, bits, len(data) // align)


def write_wav(path, y, sr, norm=False):
    """librosa.output.write_wav (0.7.1 output.py): y mono (n,) or stereo (2, n); float data is written as
    32/64-bit float WAVE unchanged unless norm=True (peak-normalised to 1)."""
    if torch.is_tensor(y):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if not np.issubdtype(y.dtype, np.floating):
        raise ValueError("Audio data must be floating-point")          # librosa.util.valid_audio
    if y.ndim not in (1, 2) or not np.isfinite(y).all():
        raise ValueError("Audio buffer is not finite everywhere or has a bad shape")
    wav = y
    if norm:
        peak = np.max(np.abs(y)) if y.size else 0.0
        wav = y / peak if peak > np.finfo(y.dtype).tiny else y
    if wav.ndim > 1 and wav.shape[0] == 2:
        wav = wav.T
    with open(path, "wb") as fp:
        fp.write(wave_bytes(wav, sr))
