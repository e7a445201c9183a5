"""sos_pcm_encode_dither_batch (csrc/pcm_io.hip, csrc/dither_core.h) and audio_io.encode_batch_device(dither=) /
pcm_encode_device against the numpy restatement tests/dither_reference.py.  The rule is exact (integers, and float64 sums rounded
once), so EVERY comparison below is equality of bytes and counts: there is no tolerance in this file.
ONE ragged group, encoded once per (format, kind) and shared by the tests (FILES below): channels 1, 2, 3 and 5, so that a
thread's four interleaved elements straddle frames; lengths 0, 1, 3, 4, 5 and 1001; odd element counts ahead of the others, so that
s16 files start off a 4-element boundary and s24 files at all four byte positions of a dword; frames above the plane's length
(dithered zero-fill) and below it (crop); pcm_reference.edge_values for the counts; one mono file of 1 100 000 samples, past the
1024 x 256 x 4 elements one sweep of the grid covers; first frames 1, 2, 3, 2^34 - 3 (the counter's low word carries into its
high word inside the file) and the largest a file may have, 2^62 - frames; keys 0 .. 2^32 - 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import dither_reference as D
import pcm_reference as R
from test_dither_host_cpu import (test_c_refuses_a_key_or_first_frame_out_of_range, test_c_refuses_another_kind,  # noqa: F401
                                  test_c_refuses_the_formats_without_dither, test_c_refuses_what_the_plain_encode_refuses,
                                  test_python_refuses_before_any_launch, test_the_packet_form_checks_its_own_arguments)
# (the refusals: host code only, collected here a second time so that they also run beside the kernels)

pytestmark = pytest.mark.gpu
SEED = (0xC0FFEE << 32) | 0x1234                                # both key words in use
BIG = 1100000
# channels, plane length, frames to write, first absolute frame, key
FILES = ((1, 1, 1, 0, 0), (1, 5, 5, 1, 1), (2, 3, 3, 2, 2), (3, 1001, 1001, 3, 3), (5, 4, 4, 2**34 - 3, (1 << 32) - 1), (1, 0, 0, 0, 5),
         (2, 1001, 1010, 2**34 - 3, 6), (1, 1001, 600, 1, 7), (1, 0, 40, 5, 8), (3, 5, 9, 2**34 - 3, 9), (1, BIG, BIG + 3, 3, 10),
         (5, 1001, 1001, 1, 11), (2, 4, 4, 2**62 - 4, 12), (1, 3, 2, 2, 4))
SENTINEL = 0xA5
CASES = [(fmt, kind) for fmt in D.FORMATS for kind in D.KINDS]


def _plane(ch, n, fmt, rng, k):
    """(channels, n) float32: a third within a few LSB of zero (where dither matters), the rest over [-1.2, 1.2], the rule's tie
    and edge values among them."""
    p = rng.uniform(-1.2, 1.2, size=(ch, n)).astype(np.float32)
    flat = p.reshape(-1)
    flat[1::3] *= np.float32(4.0 / R.scale(fmt))
    edge = R.edge_values(fmt)
    step = 5 if flat.size >= 110 else 1
    pos = np.arange(0, flat.size, step)
    flat[pos] = edge[(pos // step + k) % len(edge)]
    return p


@pytest.fixture(scope="module")
def group():
    """Per format: the planes on the host and the device; per (format, kind): the reference's bytes and counts and the kernels',
    each computed once and left unchanged."""
    from sos_amd import audio_io
    rng = np.random.default_rng(59)
    out = dict(frames=[f[2] for f in FILES], frame0=[f[3] for f in FILES], keys=[f[4] for f in FILES])
    for fmt in D.FORMATS:
        host = [_plane(ch, n, fmt, rng, k) for k, (ch, n, _, _, _) in enumerate(FILES)]
        out[fmt] = dict(host=host, dev=[torch.from_numpy(p).cuda() for p in host])
        for kind in D.KINDS:
            ref = [D.encode(p, fmt, fr, kind, SEED, key, f0) for p, (_, _, fr, f0, key) in zip(host, FILES)]
            got = audio_io.encode_batch_device(out[fmt]["dev"], fmt, frames=out["frames"], dither=kind, seed=SEED, keys=out["keys"],
                                               frame0=out["frame0"])
            out[fmt, kind] = dict(ref=ref, data=got[0].cpu().numpy(), offsets=got[1], clipped=got[2].cpu().tolist())
    return out


def _first_difference(got, want):
    want = np.frombuffer(want, dtype=np.uint8)
    if got.size != want.size:
        return "%d bytes, the reference has %d" % (got.size, want.size)
    bad = np.flatnonzero(got != want)
    return None if not bad.size else "%d bytes differ, the first at %d" % (bad.size, bad[0])


@pytest.mark.parametrize("fmt,kind", CASES)
def test_group_bytes_and_counts_are_the_reference(fmt, kind, group):
    g = group[fmt, kind]
    want_off = np.cumsum([0] + [fr * ch * R.WIDTH[fmt] for ch, _, fr, _, _ in FILES])
    assert np.array_equal(g["offsets"], want_off)
    if fmt == "s16":
        assert any((o // 2) % 4 for o in want_off[:-1])         # files off a 4-element boundary
    if fmt == "s24":
        assert {int(o) % 4 for o in want_off[:-1]} == {0, 1, 2, 3}      # and at every byte of a dword
    for k, (data, _) in enumerate(g["ref"]):
        assert _first_difference(g["data"][want_off[k]:want_off[k + 1]], data) is None, (k, FILES[k])
    assert g["clipped"] == [r[1] for r in g["ref"]] and sum(g["clipped"]) > 0
    plain = b"".join(R.encode(p, fmt, fr)[0] for p, fr in zip(group[fmt]["host"], group["frames"]))
    assert g["data"].tobytes() != plain                        # it is not the undithered encode


@pytest.mark.parametrize("fmt,kind", CASES)
def test_the_zero_fill_is_dithered(fmt, kind, group):
    """File 8 has no plane sample at all: forty frames of dither around zero, not forty zeros."""
    data, clipped = group[fmt, kind]["ref"][8]
    q = R.unpack(data, fmt, 1).reshape(-1) - (128 if fmt == "u8" else 0)
    assert clipped == 0 and set(q.tolist()) <= {-1, 0, 1} and q.any()


@pytest.mark.parametrize("fmt,kind", CASES)
def test_a_file_alone_has_the_bytes_it_has_in_the_group(fmt, kind, group):
    """Alone, a file starts on aligned addresses on both sides (the 16-byte accesses), shares its launch with nobody and has
    another grid: the mono file past one sweep of the grid, the interleaved ones, the zero-fill, the crop."""
    from sos_amd import audio_io
    g = group[fmt, kind]
    for k in (10, 3, 6, 7, 9, 12):
        _, _, fr, f0, key = FILES[k]
        data, _, clipped = audio_io.encode_batch_device([group[fmt]["dev"][k]], fmt, frames=[fr], dither=kind, seed=SEED, keys=[key],
                                                        frame0=[f0])
        assert _first_difference(data.cpu().numpy(), g["ref"][k][0]) is None, k
        assert clipped.cpu().tolist() == [g["ref"][k][1]]


@pytest.mark.parametrize("fmt,kind", CASES)
def test_packets_concatenate_to_the_one_call_encode(fmt, kind):
    from sos_amd import audio_io
    rng = np.random.default_rng(61)
    sizes = [1, 7, 160, 4099, 4099, 160, 7, 1, 160]
    x = _plane(1, sum(sizes), fmt, rng, 0)
    dev = torch.from_numpy(x[0]).cuda()
    for start in (0, 2**34 - 3):
        whole, count = audio_io.pcm_encode_device(dev, fmt, kind, SEED, 77, start)
        want, want_count = D.encode(x, fmt, None, kind, SEED, 77, start)
        assert _first_difference(whole.cpu().numpy(), want) is None and count.cpu().tolist() == [want_count]
        parts, counts, at = [], 0, 0
        for n in sizes:                                          # the caller's only state: the frames sent so far
            data, c = audio_io.pcm_encode_device(dev[at:at + n], fmt, kind, SEED, 77, start + at)
            parts.append(data)
            counts += int(c)
            at += n
        assert torch.equal(torch.cat(parts), whole) and counts == want_count


@pytest.mark.parametrize("fmt,kind", CASES)
def test_two_calls_agree_and_another_seed_key_or_first_frame_differs(fmt, kind, group):
    from sos_amd import audio_io
    dev, k = group[fmt]["dev"][3:4], FILES[3]
    args = dict(frames=[k[2]], dither=kind, seed=SEED, keys=[k[4]], frame0=[k[3]])
    a, b = audio_io.encode_batch_device(dev, fmt, **args), audio_io.encode_batch_device(dev, fmt, **args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for change in (dict(seed=SEED + 1), dict(seed=SEED ^ (1 << 40)), dict(keys=[k[4] + 1]), dict(frame0=[k[3] + 1]),
                   dict(dither=[d for d in D.KINDS if d != kind][0])):
        other = audio_io.encode_batch_device(dev, fmt, **dict(args, **change))
        assert not torch.equal(other[0], a[0]), change
    default = audio_io.encode_batch_device(group[fmt]["dev"][:4], fmt, dither=kind, seed=SEED)    # keys: positions, frame0: 0
    want = b"".join(D.encode(p, fmt, None, kind, SEED, j, 0)[0] for j, p in enumerate(group[fmt]["host"][:4]))
    assert default[0].cpu().numpy().tobytes() == want


@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32", "f32", "ulaw"])
def test_dither_none_is_the_call_without_the_argument(fmt, group):
    from sos_amd import audio_io
    dev, frames = group["s16"]["dev"][:10], group["frames"][:10]
    a = audio_io.encode_batch_device(dev, fmt, frames=frames)
    b = audio_io.encode_batch_device(dev, fmt, frames=frames, dither=None, seed=9, keys=[3] * 10, frame0=[5] * 10)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and torch.equal(a[2], b[2])
    if fmt in R.WIDTH:
        assert a[0].cpu().numpy().tobytes() == b"".join(R.encode(p, fmt, fr)[0] for p, fr in zip(group["s16"]["host"], frames))
        x, n = audio_io.pcm_encode_device(dev[3][0], fmt)
        assert x.cpu().numpy().tobytes() == R.encode(group["s16"]["host"][3][:1], fmt)[0] and n.shape == (1,)


@pytest.mark.parametrize("fmt,lead", [("s16", 2), ("s24", 1), ("s24", 2), ("s24", 3), ("u8", 1), ("u8", 0)])
def test_the_entry_point_leaves_the_sentinels_wherever_the_output_starts(fmt, lead, group):
    """The C entry point itself, the output between sentinel bytes and `lead` bytes past a 256-byte boundary; the small files
    (without the mono file of 1.1 M samples), 'highpass' (it reads one frame ahead, never one byte)."""
    from sos_amd import _lib as L
    from sos_amd import audio_io
    keep = [k for k in range(len(FILES)) if k != 10]
    planes = [group[fmt]["host"][k] for k in keep]
    ch, avail, frames = (np.asarray([FILES[k][c] for k in keep], dtype=np.int64) for c in (0, 1, 2))
    src, dst = np.cumsum(ch * avail) - ch * avail, np.cumsum(ch * frames) - ch * frames
    tab = np.ascontiguousarray(np.stack([src, avail, ch, frames, dst, [FILES[k][4] for k in keep], [FILES[k][3] for k in keep]], axis=1),
                               dtype=np.int64)
    flat = torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).cuda()
    nbytes, pad = int((ch * frames).sum()) * R.WIDTH[fmt], 256
    out = torch.full((pad + lead + nbytes + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    counts = torch.full((len(keep) + 2,), -9, dtype=torch.int64, device="cuda")
    rc = L.lib().sos_pcm_encode_dither_batch(L.ptr(flat), L.ptr(torch.from_numpy(tab).cuda()), tab.ctypes.data_as(C.c_void_p), len(keep),
                                             audio_io.ENCODINGS[fmt][0], audio_io.DITHER["highpass"], SEED, L.ptr(out[pad + lead:]),
                                             L.ptr(counts[1:]), L.stream_ptr())
    assert rc == 0, L.lib().sos_last_error()
    host, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert np.all(host[:pad + lead] == SENTINEL) and np.all(host[pad + lead + nbytes:] == SENTINEL), "the encode wrote outside its output"
    ref = [group[fmt, "highpass"]["ref"][k] for k in keep]
    assert host[pad + lead:pad + lead + nbytes].tobytes() == b"".join(r[0] for r in ref)
    assert counts.tolist() == [-9] + [r[1] for r in ref] + [-9]
