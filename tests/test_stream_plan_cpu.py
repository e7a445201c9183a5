"""The streaming rule on the host: pipeline.StreamPlan yields window_plan's rows without knowing the length, what it emits
tiles the output, tests/stream_reference.py equals window_reference.stitch exactly, and the three entry points of
csrc/stream_window.hip refuse on the host before any launch (dummy pointers that are never followed, as in
test_window_planes_cpu.py): every refusal is -22 (SOS_EINVAL) and names the row."""
import ctypes as C

import numpy as np
import pytest

import stream_reference as SR
import window_reference as R

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
# around 1, 2, 3 and 8 cores: multiples of the core, of the hop and neither, just below and above (k + 2) core
LENGTHS = sorted({m * CORE + d for m in (1, 2, 3, 8) for d in (-HOP - 1, -HOP, -3, -2, -1, 0, 1, 2, 3, HOP - 1, HOP, HOP + 1, 5 * HOP + 77)}
                 | {64 * HOP, 64 * HOP + 1, 150 * HOP + 31})


def _chunkings(n, rng):
    """Sizes that sum to n: one chunk, random sizes from one sample to several windows, and single samples around every multiple
    of the core."""
    yield [n]
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.choice([1, 7, 100, 1000, CORE - 1, CORE, 3 * CORE + 5])), n - sum(sizes)))
    yield sizes
    cuts = sorted({c for j in range(1, n // CORE + 2) for c in range(j * CORE - 2, j * CORE + 3) if 0 < c < n})
    yield [b - a for a, b in zip([0] + cuts, cuts + [n])]


def test_feed_and_close_yield_window_plans_rows_and_the_emitted_ranges_tile_the_output():
    from sos_amd import pipeline
    rng = np.random.default_rng(3)
    for n in LENGTHS:
        want = pipeline.window_plan([n], CORE, CONTEXT)
        assert np.array_equal(want[:, [1, 2, 4, 5]], [[w.start, w.samples, w.core_start, w.core_end] for w in R.plan([n], CORE, CONTEXT)])
        for sizes in _chunkings(n, rng):
            plan = pipeline.StreamPlan(CORE, CONTEXT)
            rows, pending = [], 0
            for c in sizes:
                got = plan.feed(c)
                assert got.shape[1:] == (10,) and got.dtype == np.int64
                rows.extend(got)
                pending = max(pending, plan.pending)
            rows.extend(plan.close())
            assert np.array_equal(np.asarray(rows), want), (n, sizes[:8])
            assert pending < 2 * CORE + CONTEXT and plan.n_in == plan.k == 0
            ranges = [plan.emitted(r) for r in rows]
            assert ranges[0][0] == 0 and ranges[-1][1] == HOP * (n // HOP)
            assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(ranges, ranges[1:])) and ranges[-1][0] < ranges[-1][1]


def test_the_plan_refuses_what_window_plan_refuses():
    from sos_amd import pipeline
    for core, context in ((CORE, CORE // 2 + HOP), (40 * HOP, 8 * HOP), (-1, 0)):
        with pytest.raises(ValueError):
            pipeline.StreamPlan(core, context)
    plan = pipeline.StreamPlan(CORE, CONTEXT)
    plan.feed(64 * HOP - 1)
    with pytest.raises(ValueError, match="at least 65 STFT frames"):
        plan.close()
    assert len(plan.feed(64 * HOP)) == 0 and len(plan.close()) == 1        # a new stream afterwards


@pytest.mark.parametrize("extra", [0, 5, 4 * CORE])
def test_the_stream_reference_is_the_stitch_of_the_whole_recording(extra):
    rng = np.random.default_rng(5 + extra)
    for n in LENGTHS:
        x = rng.standard_normal(n)
        wins = R.plan([n], CORE, CONTEXT)
        rows = [rng.standard_normal(HOP * (w.samples // HOP)) for w in wins]
        want, _ = R.stitch(wins, rows, CONTEXT)
        own, _ = R.stitch(wins, [x[w.start:w.start + HOP * (w.samples // HOP)] for w in wins], CONTEXT)
        for sizes in list(_chunkings(n, rng))[1:]:
            run = SR.simulate(x, sizes, CORE, CONTEXT, capacity=2 * CORE + CONTEXT + extra, rows=rows)
            assert run.wins == wins and np.array_equal(run.out, want)
            assert all(np.array_equal(s, x[w.start:w.start + w.samples]) for s, w in zip(run.staged, wins))
            assert run.emitted[0][0] == 0 and run.emitted[-1][1] == len(want) and all(a[1] == b[0] for a, b in zip(run.emitted, run.emitted[1:]))
        assert np.array_equal(SR.simulate(x, sizes, CORE, CONTEXT, capacity=2 * CORE + CONTEXT + extra).out, own)


def test_the_stream_reference_at_hop_one():
    """The geometry of tests/test_gpu_stream_window.py: core 8, context 4 and 0, every chunk size from one sample on."""
    rng = np.random.default_rng(9)
    for context in (4, 0):
        for n in list(range(1, 40)) + [100]:
            x = rng.standard_normal(n)
            wins = R.plan([n], 8, context, hop=1, min_frames=1)
            rows = [rng.standard_normal(w.samples) for w in wins]
            want, _ = R.stitch(wins, rows, context)
            for chunk in (1, 3, 7, 40):
                sizes = [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])
                for cap in (16 + context, 16 + context + 5):
                    run = SR.simulate(x, sizes, 8, context, capacity=cap, rows=rows, hop=1, min_frames=1)
                    assert run.wins == wins and np.array_equal(run.out, want)


P, NULL = C.c_void_p(1 << 20), C.c_void_p(0)


def _refusals(fn, who, cases):
    from sos_amd import _lib as L
    h = L.lib()
    for args, want in cases:
        rc = fn(h, **args)
        msg = h.sos_last_error().decode()
        assert rc == -22 and want in msg and msg.startswith(who + ": "), (args, want, rc, msg)


def _tab(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int64))


def test_the_push_refuses_on_the_host_and_names_the_row():
    good = [[0, 0, 10, 0], [2, 10, 20, 45], [1, 30, 0, 7]]

    def call(h, t=good, flat=P, ring=P, dev=P, host=True, total=30, nrows=None, slots=3, cap=20):
        t = _tab(t)
        return h.sos_stream_push_f32(flat, total, dev, t.ctypes.data if host else None, len(t) if nrows is None else nrows, ring,
                                     slots, cap, None)

    def changed(i, col, value):
        t = _tab(good)
        t[i, col] = value
        return t

    _refusals(call, "sos_stream_push_f32", [
        (dict(flat=NULL), "null pointer"), (dict(ring=NULL), "null pointer"), (dict(dev=NULL), "null pointer"),
        (dict(host=False), "null pointer"), (dict(nrows=0), "rows, got 0"), (dict(nrows=65536), "rows, got 65536"),
        (dict(slots=0), "slots, got 0"), (dict(slots=65536), "slots, got 65536"), (dict(cap=0), "a ring of 0 samples"),
        (dict(total=-1), "a buffer of -1 samples"),
        (dict(t=changed(1, 0, 3)), "row 1 names slot 3 of 3"), (dict(t=changed(1, 0, -1)), "row 1 names slot -1 of 3"),
        (dict(slots=2), "row 1 names slot 2 of 2"),
        (dict(t=changed(2, 0, 0)), "row 2 names slot 0, which an earlier row"),
        (dict(t=changed(1, 2, 21)), "row 1 has 21 samples (a ring holds 20)"), (dict(cap=19), "row 1 has 20 samples (a ring holds 19)"),
        (dict(t=changed(1, 3, -1)), "row 1 writes at the stream position -1"),
        (dict(t=changed(0, 1, -1)), "row 0 (samples -1 + 10) lies outside the 30 samples"),
        (dict(t=changed(1, 1, 11)), "row 1 (samples 11 + 20) lies outside the 30 samples"),
        (dict(t=changed(2, 2, -1)), "row 2 (samples 30 + -1) lies outside"), (dict(total=29), "row 1 "),
    ])


def test_the_stage_refuses_on_the_host_and_names_the_row():
    good = [[0, 0, 12], [2, 45, 16], [2, 45, 16], [1, 7, 0]]           # a slot may be staged twice: nothing is written to it

    def call(h, t=good, ring=P, rows=P, dev=P, host=True, nwin=None, slots=3, cap=20, stride=16):
        t = _tab(t)
        return h.sos_stream_stage_f32(ring, slots, cap, dev, t.ctypes.data if host else None, len(t) if nwin is None else nwin,
                                      stride, rows, None)

    def changed(i, col, value):
        t = _tab(good)
        t[i, col] = value
        return t

    _refusals(call, "sos_stream_stage_f32", [
        (dict(ring=NULL), "null pointer"), (dict(rows=NULL), "null pointer"), (dict(dev=NULL), "null pointer"),
        (dict(host=False), "null pointer"), (dict(nwin=0), "rows, got 0"), (dict(slots=0), "slots, got 0"),
        (dict(cap=0), "a ring of 0 samples"), (dict(stride=0), "stride 0"),
        (dict(t=changed(3, 0, 3)), "row 3 names slot 3 of 3"), (dict(t=changed(0, 0, -1)), "row 0 names slot -1 of 3"),
        (dict(t=changed(1, 2, 17)), "row 1 has 17 samples (stride 16, a ring holds 20)"),
        (dict(stride=24, t=changed(1, 2, 21)), "row 1 has 21 samples (stride 24, a ring holds 20)"),
        (dict(cap=15), "row 1 has 16 samples (stride 16, a ring holds 15)"), (dict(t=changed(0, 2, -1)), "row 0 has -1 samples"),
        (dict(t=changed(2, 1, -1)), "row 2 starts at the stream position -1"),
    ])


def test_the_stitch_refuses_on_the_host_and_names_the_row():
    # {slot, row, window start, samples, core start, core end, flags, parity}: a first, an inner and a last window at core 8 / context 4
    good = [[0, 0, 0, 12, 0, 8, 2, 0], [2, 1, 4, 16, 8, 16, 3, 1], [1, 2, 12, 11, 16, 23, 1, 0]]

    def call(h, t=good, rows=P, out=P, tail=P, dev=P, host=True, n_rows=3, stride=16, nwin=None, slots=3, context=4, out_stride=11):
        t = _tab(t)
        return h.sos_stream_stitch_f32(rows, n_rows, stride, dev, t.ctypes.data if host else None, len(t) if nwin is None else nwin,
                                       slots, context, tail, out, out_stride, None)

    def changed(i, col, value):
        t = _tab(good)
        t[i, col] = value
        return t

    _refusals(call, "sos_stream_stitch_f32", [
        (dict(rows=NULL), "null pointer"), (dict(out=NULL), "null pointer"), (dict(tail=NULL), "null pointer"),
        (dict(dev=NULL), "null pointer"), (dict(host=False), "null pointer"), (dict(nwin=0), "rows, got 0"),
        (dict(nwin=65536), "rows, got 65536"), (dict(slots=0), "slots, got 0"), (dict(slots=65536), "slots, got 65536"),
        (dict(stride=0), "bad args"), (dict(n_rows=0), "bad args"), (dict(out_stride=0), "bad args"),
        (dict(context=-1), "context -1"), (dict(context=(1 << 22) + 1), "context 4194305, 0 .. 4194304"),
        (dict(t=changed(1, 0, 3)), "row 1 names slot 3 of 3"), (dict(t=changed(1, 0, -1)), "row 1 names slot -1 of 3"),
        (dict(slots=2), "row 1 names slot 2 of 2"),
        (dict(t=changed(2, 0, 0)), "row 2 names slot 0, which an earlier row"),
        (dict(t=changed(1, 1, 3)), "row 1 names a row outside the rows"), (dict(n_rows=2), "row 2 names a row outside the rows"),
        (dict(t=changed(1, 3, 17)), "row 1 has more samples than the stride"), (dict(t=changed(0, 3, -1)), "row 0 has more samples"),
        (dict(t=changed(1, 5, 21)), "row 1 has a core outside its own samples"),
        (dict(t=changed(1, 2, 9)), "row 1 has a core outside its own samples"),
        (dict(t=changed(2, 4, 24)), "row 2 has a core outside its own samples"),
        (dict(t=changed(1, 2, -1)), "row 1 has a core outside its own samples"),
        (dict(t=changed(1, 2, 5)), "row 1 has an overlap outside its own samples"),        # before the core: 3 < context
        (dict(t=changed(1, 3, 15)), "row 1 has an overlap outside its own samples"),       # after it
        (dict(t=changed(0, 3, 11)), "row 0 has an overlap outside its own samples"),
        (dict(t=changed(2, 5, 19)), "row 2 blends over more context than its core holds"),
        (dict(context=5), "row 0 has an overlap outside its own samples"),
        (dict(t=changed(1, 6, 4)), "row 1 has flags outside"), (dict(t=changed(1, 6, -1)), "row 1 has flags outside"),
        (dict(t=changed(1, 7, 2)), "row 1 has flags outside 0 .. 3 or a parity outside 0 .. 1"),
        (dict(out_stride=10), "row 2 emits more samples than the output stride"),
    ])


def test_the_abi_version_is_unchanged_and_the_entry_points_are_declared():
    from sos_amd import _lib as L
    assert L.lib().sos_abi_version() == 10
    assert all(name in L.SIGNATURES for name in ("sos_stream_push_f32", "sos_stream_stage_f32", "sos_stream_stitch_f32"))
