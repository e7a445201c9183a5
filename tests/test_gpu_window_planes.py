"""sos_window_stitch_planes_f32 (csrc/ragged_window.hip; tools.window_stitch_planes): several signals of one plan stitched in one
launch.  The yardstick is the one-plane call, sos_window_stitch_f32, which tests/test_gpu_window.py holds against the float64
restatement: every plane must carry ITS bits, wherever the destination table puts it."""
import numpy as np
import pytest
import torch

import window_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
SPARE = 16


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _case(ns, core, context, planes, residue, seed):
    """Plan and table of `ns` at hop 1, and random rows (planes, windows, stride) with stride % 4 == residue."""
    wins = R.plan(ns, core, context, hop=1, min_frames=1)
    tab = R.table(wins, ns, hop=1)
    stride = max(w.samples for w in wins) + 1
    stride += (residue - stride) % 4
    rows = np.random.default_rng(seed).standard_normal((planes, len(wins), stride)).astype(np.float32)
    return wins, tab, rows


def _subtable(tab, idx, out_shift=0, recording=None):
    """Rows `idx` of a table, in that order, as a table of their own: neighbours renumbered, outputs moved by -out_shift."""
    new = {int(w): i for i, w in enumerate(idx)}
    sub = tab[np.asarray(idx)].copy()
    sub[:, 3] -= out_shift
    if recording is not None:
        sub[:, 0] = recording
    for col in (8, 9):
        sub[:, col] = [new[int(v)] if v >= 0 else -1 for v in sub[:, col]]
    return np.ascontiguousarray(sub)


def _one_plane(d_rows, tab, context):
    """What sos_window_stitch_f32 gives for each plane alone: (planes, total), on the host."""
    from sos_amd import tools
    return np.stack([tools.window_stitch(d_rows[q], tab, context).cpu().numpy() for q in range(d_rows.shape[0])])


CASES = [([31, 5, 4097, 16, 100], 8, 4), ([31, 5, 4097, 16, 100], 8, 0), ([5000, 2999, 12345, 2000], 1000, 300),
         ([5000, 2999, 12345, 2000], 1001, 1)]


@pytest.mark.parametrize("planes", [1, 4, 6])
@pytest.mark.parametrize("residue", [0, 3], ids=["stride%4=0", "stride%4=3"])
@pytest.mark.parametrize("ns,core,context", CASES, ids=["core8-context4", "core8-cut", "core1000-context300", "core1001-context1"])
def test_plane_major_planes_are_the_one_plane_stitches(ns, core, context, residue, planes):
    from sos_amd import tools
    wins, tab, rows = _case(ns, core, context, planes, residue, seed=core + context + planes)
    assert rows.shape[2] % 4 == residue
    d_rows = torch.from_numpy(rows).cuda()
    got = tools.window_stitch_planes(d_rows, tab, context).cpu().numpy()
    assert got.shape == (planes, sum(ns))
    want = _one_plane(d_rows, tab, context)
    for q in range(planes):
        assert _same_bits(got[q], want[q]), q
    if planes > 1:
        assert not _same_bits(got[0], got[1])


def _file_major(ns, planes):
    """{base, pitch} per recording: pitches 0 .. 3 samples above the lengths, bases at every residue mod 4; and the total."""
    recs, cursor = [], 0
    for r, n in enumerate(ns):
        base = cursor + (r - cursor) % 4
        recs.append((base, n + (3 - r) % 4))
        cursor = base + planes * recs[-1][1]
    return np.asarray(recs, dtype=np.int64), cursor


def _raw(d_rows, tab, d_tab, context, recs, d_recs, out_total, out):
    from sos_amd import _lib as L
    return L.lib().sos_window_stitch_planes_f32(L.ptr(d_rows), d_rows.shape[0], d_rows.shape[1], d_rows.shape[2], L.ptr(d_tab),
                                                tab.ctypes.data, len(tab), context, L.ptr(d_recs), recs.ctypes.data, len(recs),
                                                out_total, L.ptr(out), L.stream_ptr())


@pytest.mark.parametrize("planes", [1, 4, 6])
@pytest.mark.parametrize("residue", [0, 3], ids=["stride%4=0", "stride%4=3"])
def test_file_major_segments_are_the_plane_major_ones_and_gaps_are_left_alone(residue, planes):
    from sos_amd import tools
    ns = [5001, 2999, 12345, 2000]
    wins, tab, rows = _case(ns, 1000, 300, planes, residue, seed=21 + planes)
    d_rows = torch.from_numpy(rows).cuda()
    major = tools.window_stitch_planes(d_rows, tab, 300).cpu().numpy()
    recs, out_total = _file_major(ns, planes)
    assert sorted(int(b) % 4 for b in recs[:, 0]) == [0, 1, 2, 3] and sorted(int(p - n) for p, n in zip(recs[:, 1], ns)) == [0, 1, 2, 3]
    out = torch.full((out_total + SPARE,), SENTINEL, device="cuda")
    d_tab, d_recs = torch.from_numpy(tab).cuda(), torch.from_numpy(recs).cuda()
    assert _raw(d_rows, tab, d_tab, 300, recs, d_recs, out_total, out) == 0
    got = out.cpu().numpy()
    written = np.zeros(out_total + SPARE, dtype=bool)
    starts = np.cumsum(ns) - ns
    for r, n in enumerate(ns):
        for q in range(planes):
            at = int(recs[r, 0] + q * recs[r, 1])
            assert _same_bits(got[at:at + n], major[q, starts[r]:starts[r] + n]), (r, q)
            assert not written[at:at + n].any()
            written[at:at + n] = True
    assert (~written).sum() > SPARE and (got[~written] == SENTINEL).all()                # the gaps and what lies behind the buffer
    # the package's call: the same segments, zero where nothing is written
    flat = tools.window_stitch_planes(d_rows, tab, 300, recs=recs, out_total=out_total).cpu().numpy()
    assert flat.shape == (out_total,) and _same_bits(flat[written[:out_total]], got[:out_total][written[:out_total]])
    assert not flat[~written[:out_total]].any()


def test_same_bits_permuted_with_moved_rows_and_alone():
    from sos_amd import tools
    ns, planes, context = [5001, 2999, 12345, 2000], 4, 300
    wins, tab, rows = _case(ns, 1000, context, planes, 3, seed=31)
    d_rows = torch.from_numpy(rows).cuda()
    batch = tools.window_stitch_planes(d_rows, tab, context).cpu().numpy()
    perm = np.random.default_rng(32).permutation(len(wins))
    assert _same_bits(tools.window_stitch_planes(d_rows, _subtable(tab, perm), context).cpu().numpy(), batch)
    # the rows in another order and at another stride: row indices are the table's business
    order = np.random.default_rng(33).permutation(len(wins))
    moved = np.zeros((planes, len(wins), rows.shape[2] + 1), np.float32)
    moved[:, order, :-1] = rows
    tab2 = tab.copy()
    tab2[:, 7] = order
    assert _same_bits(tools.window_stitch_planes(torch.from_numpy(moved).cuda(), tab2, context).cpu().numpy(), batch)
    # a recording alone, with recs of its own: plane-major, and file-major at an odd base
    starts = np.cumsum(ns) - ns
    for r, n in enumerate(ns):
        idx = [i for i, w in enumerate(wins) if w.recording == r]
        sub = _subtable(tab, idx, starts[r], recording=0)
        alone = tools.window_stitch_planes(d_rows, sub, context).cpu().numpy()
        assert _same_bits(alone, batch[:, starts[r]:starts[r] + n]), r
        flat = tools.window_stitch_planes(d_rows, sub, context, recs=[(1, n + 2)], out_total=1 + planes * (n + 2)).cpu().numpy()
        for q in range(planes):
            assert _same_bits(flat[1 + q * (n + 2):1 + q * (n + 2) + n], alone[q]), (r, q)


def test_the_kernel_skips_a_window_whose_device_entry_leaves_the_hosts_sizes():
    """The device rule: the host tables are correct, a DEVICE table differs in one entry.  The call succeeds, that window's core
    keeps the sentinel in every plane, everything else is what the unaltered call gives, nothing behind the buffers is written
    (spare elements behind every buffer keep a wrongly followed entry inside allocated memory)."""
    ns, planes, context = [31, 5, 100], 4, 4
    wins, tab, rows = _case(ns, 8, context, planes, 0, seed=41)
    W, total, nrec = len(wins), sum(ns), len(ns)
    assert W == 16 and wins[3].recording == 1 and wins[2].recording == 0
    recs = np.ascontiguousarray(np.stack([np.cumsum(ns) - ns, np.full(nrec, total)], axis=1).astype(np.int64))
    out_total = planes * total
    d_rows = torch.from_numpy(np.concatenate([rows.reshape(-1), np.zeros(SPARE + rows.shape[2], np.float32)])).cuda()
    d_rows3 = d_rows[:rows.size].view(rows.shape)

    def stitch(tab_change=None, rec_change=None):
        d_tab = torch.from_numpy(np.concatenate([tab.reshape(-1), np.zeros(SPARE, np.int64)])).cuda()
        d_recs = torch.from_numpy(np.concatenate([recs.reshape(-1), np.zeros(SPARE, np.int64)])).cuda()
        if tab_change:
            d_tab[tab_change[0] * 10 + tab_change[1]] = int(tab_change[2])
        if rec_change:
            d_recs[rec_change[0] * 2 + rec_change[1]] = int(rec_change[2])
        out = torch.full((out_total + SPARE,), SENTINEL, device="cuda")
        assert _raw(d_rows3, tab, d_tab, context, recs, d_recs, out_total, out) == 0
        return out.cpu().numpy()

    base = stitch()
    assert not (base[:out_total] == SENTINEL).any() and (base[out_total:] == SENTINEL).all()
    # window 3 is a recording of its own (no window reads its entry as a neighbour's); window 2 is the last of three: its
    # `previous` is read by itself only
    for w, tab_change, rec_change in ((3, (3, 7, W), None),                  # a row outside n_rows
                                      (3, (3, 0, nrec), None), (3, (3, 0, -1), None),       # a recording outside nrec
                                      (3, None, (1, 0, out_total)), (3, None, (1, 0, out_total - 4)),      # a base past out_total, and one whose last plane leaves it
                                      (3, None, (1, 1, 4)),                  # a pitch below the core's end
                                      (2, (2, 8, W), None), (2, (2, 8, 4), None)):          # a neighbour outside the table, and another recording's window
        got = stitch(tab_change, rec_change)
        lo, hi = int(tab[w, 3] + tab[w, 4] - tab[w, 6]), int(tab[w, 3] + tab[w, 5] - tab[w, 6])
        skipped = np.zeros(out_total + SPARE, dtype=bool)
        for q in range(planes):
            skipped[q * total + lo:q * total + hi] = True
        assert (got[skipped] == SENTINEL).all() and (got[out_total:] == SENTINEL).all(), (w, tab_change, rec_change)
        assert _same_bits(got[~skipped], base[~skipped]), (w, tab_change, rec_change)
