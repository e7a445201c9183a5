"""The three kernels of csrc/stream_window.hip alone (no networks, hop 1): chunks pushed into rings that wrap several times, windows
staged out of them and random rows stitched call after call give, bit for bit, what tools.window_stage / tools.window_stitch
give for the complete recordings.  Plans: tests/stream_reference.py and tests/window_reference.py."""
import numpy as np
import pytest
import torch

import stream_reference as SR
import window_reference as R

pytestmark = pytest.mark.gpu

CORE = 8
NS = [5, 31, 100]                   # one window, three windows, twelve windows at core 8 and hop 1
STRIDE = 24                         # >= core + 2 context, a multiple of four
CHUNKS = (1, 3, 7, 40)


@pytest.fixture(scope="module")
def data():
    """The recordings and one row of random values per window (context 4 and 0 share them).  Never modified."""
    rng = np.random.default_rng(21)
    return [rng.standard_normal(n).astype(np.float32) for n in NS], rng.standard_normal((16, STRIDE)).astype(np.float32)


def _session(data, rows_all, context, extra, slot_of, n_slots, recs=(0, 1, 2), reverse=False):
    """The recordings `recs` streamed through slots slot_of[r] of a session of n_slots rings of 2 core + context + extra samples:
    every call brings each stream its next chunk (sizes 1, 3, 7, 40 in turn, each stream at its own phase; a finished stream an
    empty one), larger than the free ring in pieces.  The windows' rows are rows_all[first window of the recording + k].
    -> per recording: (the staged rows, the emitted samples)."""
    from sos_amd import tools
    cap = 2 * CORE + context + extra
    ring = torch.zeros((n_slots, cap), device="cuda")
    tail = torch.full((n_slots, 2, max(2 * context, 1)), np.nan, device="cuda")
    d_rows = torch.from_numpy(rows_all).cuda()
    first = np.cumsum([0] + [len(R.plan([n], CORE, context, hop=1, min_frames=1)) for n in NS])
    plans = {r: SR.Plan(CORE, context, hop=1, min_frames=1) for r in recs}
    parity, fed = {r: 0 for r in recs}, {r: 0 for r in recs}
    staged, outs = {r: [] for r in recs}, {r: [] for r in recs}

    def step(items):                                            # at most one window (r, k, Window, last) per recording
        items = items[::-1] if reverse else items
        st = tools.stream_stage(ring, [(slot_of[r], w.start, w.samples) for r, _, w, _ in items], STRIDE)
        table = [(slot_of[r], first[r] + k, w.start, w.samples, w.core_start, w.core_end, (1 if k else 0) | (0 if last else 2), parity[r])
                 for r, k, w, last in items]
        out, lens = tools.stream_stitch(d_rows, table, context, tail)
        assert lens == [b - a for a, b in (SR.emitted(k, w, last, context) for _, k, w, last in items)]
        for i, (r, k, w, last) in enumerate(items):
            staged[r].append(st[i].cpu().numpy())
            outs[r].append(out[i, :lens[i]].cpu().numpy())
            parity[r] ^= 0 if last else 1

    call = 0
    while any(fed[r] < NS[r] for r in recs):
        sizes = {r: min(CHUNKS[(call + r) % 4], NS[r] - fed[r]) for r in recs}
        flat = torch.from_numpy(np.concatenate([data[r][fed[r]:fed[r] + sizes[r]] for r in recs] + [np.zeros(1, np.float32)])).cuda()
        offs = dict(zip(recs, np.cumsum([0] + [sizes[r] for r in recs])))
        while True:
            table, ready = [], []
            for r in recs:
                take = min(sizes[r], cap - (plans[r].n_in - plans[r].base()))
                table.append((slot_of[r], offs[r], take, plans[r].n_in))           # an empty chunk has a row too
                offs[r], sizes[r], fed[r] = offs[r] + take, sizes[r] - take, fed[r] + take
                ready.append([(r, k, w, False) for k, w in plans[r].feed(take)])
            tools.stream_push(flat, table[::-1] if reverse else table, ring)
            while any(ready):
                step([q.pop(0) for q in ready if q])
            if not any(sizes.values()):
                break
        call += 1
    step([(r,) + plans[r].close() + (True,) for r in recs])
    assert max(NS[r] for r in recs) >= 4 * cap                  # the longest stream's ring wrapped several times
    return {r: (staged[r], np.concatenate(outs[r])) for r in recs}


@pytest.fixture(scope="module")
def runs(data):
    """Three slots side by side, per (context, extra capacity).  Never modified."""
    return {(context, extra): _session(data[0], data[1], context, extra, {0: 0, 1: 1, 2: 2}, 3) for context in (4, 0) for extra in (0, 5)}


def _whole(data, context):
    from sos_amd import tools
    wins = R.plan(NS, CORE, context, hop=1, min_frames=1)
    tab = R.table(wins, NS, hop=1)
    flat = torch.from_numpy(np.concatenate(data[0])).cuda()
    return wins, tab, tools.window_stage(flat, tab, STRIDE).cpu().numpy(), tools.window_stitch(torch.from_numpy(data[1]).cuda(), tab, context).cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("context", [4, 0])
def test_staged_rows_are_window_stage_of_the_whole_recordings(data, runs, context, extra):
    wins, tab, want, _ = _whole(data, context)
    assert len(wins) == 16
    got = np.stack([row for r in range(3) for row in runs[context, extra][r][0]])
    assert _same_bits(got, want) and np.count_nonzero(got) == sum(w.samples for w in wins)


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("context", [4, 0])
def test_the_emitted_samples_are_window_stitch_of_the_whole_recordings(data, runs, context, extra):
    wins, tab, _, want = _whole(data, context)
    got = np.concatenate([runs[context, extra][r][1] for r in range(3)])
    assert np.isfinite(got).all() and _same_bits(got, want)
    at = 0
    for r, n in enumerate(NS):
        mine = [i for i, w in enumerate(wins) if w.recording == r]
        ws, rows = [wins[i] for i in mine], [data[1][i, :wins[i].samples] for i in mine]
        ref, blended = R.stitch(ws, rows, context)
        err, bound = np.abs(got[at:at + n].astype(np.float64) - ref), R.stitch_bound(ws, rows, context)
        print("context", context, "recording", r, "blended", int(blended.sum()), "max err / bound %.3f" % float((err[blended] / bound[blended]).max() if blended.any() else 0.0))
        assert np.all(err <= bound) and blended.sum() == (2 * context * (len(ws) - 1))
        at += n


def test_a_slots_bits_do_not_depend_on_its_neighbours_its_index_or_the_tables_order(data, runs):
    base = runs[4, 5]
    alone = _session(data[0], data[1], 4, 5, {2: 0}, 1, recs=(2,))
    moved = _session(data[0], data[1], 4, 5, {0: 4, 1: 0, 2: 3}, 5, reverse=True)
    for r in range(3):
        for other in ([alone] if r == 2 else []) + [moved]:
            assert all(_same_bits(a, b) for a, b in zip(other[r][0], base[r][0])) and _same_bits(other[r][1], base[r][1])
