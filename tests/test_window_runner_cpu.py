"""windows._run_windows, the one loop that runs a plan's windows in length groups, keeps their rows and writes plan[:, 7] (the row
a window ran in, which every stitch kernel trusts): on CPU tensors with a fake launch sequence whose rows hold the window's plan
index.  The reference is the loop as detect_long, denoise_long, the four-signal rows and the hand-off each spelled it out before
the runner existed, copied here literally (_loop_before)."""
import numpy as np
import pytest
import torch

HOP = 158
CORE, CONTEXT = 65 * HOP, 8 * HOP
NS = [CORE + 500, 3 * CORE + 300, 5 * CORE + 77]          # 1, 3 and 5 windows; the last recording ends off a hop
# 150 columns: the inner windows (core + 2 context: 82 frames) run alone, the shorter ones (69 .. 75) in pairs
CASES = [(256, 65536, None), (2, 65536, None), (1, 65536, None), (256, 150, None), (256, 65536, 4), (2, 150, 4)]


def _fake(planes, calls):
    def run_group(part, sub, m, rows):
        calls.append((list(part), sub.copy(), list(m), rows))
        w = HOP * (max(m) // HOP)
        idx = torch.tensor(part, dtype=torch.float32)
        if planes is None:
            return idx[:, None].expand(len(part), w).contiguous()
        return (idx[None, :, None] + 1000.0 * torch.arange(planes)[:, None, None]).expand(planes, len(part), w).reshape(planes * len(part), w)
    return run_group


def _loop_before(plan, max_batch, max_columns, run_group, planes):
    from sos_amd import ragged
    from sos_amd.pipeline import _length_groups
    hop = HOP
    ms, W = plan[:, 2].tolist(), len(plan)
    kept = torch.empty((W, hop * (max(ms) // hop)) if planes is None else (planes, W, hop * (max(ms) // hop)), dtype=torch.float32)
    done = 0
    for part in _length_groups(ms, min(max_batch, ragged.MAX_CLIPS), max_columns):
        m, B = [ms[i] for i in part], len(part)
        y = run_group(part, np.ascontiguousarray(plan[part]), m, range(done, done + B))
        if planes is None:
            kept[done:done + len(part), :y.shape[1]] = y
        else:
            kept[:, done:done + B, :y.shape[1]] = y.reshape(planes, B, y.shape[1])
        plan[part, 7] = np.arange(done, done + B)
        done += B
    return kept


@pytest.mark.parametrize("max_batch,max_columns,planes", CASES)
def test_the_runner_keeps_every_window_in_the_row_column_7_names(max_batch, max_columns, planes):
    from sos_amd import ragged, transform, windows
    from sos_amd.pipeline import _length_groups
    assert transform.HOP_LENGTH == HOP
    plan = windows.window_plan(NS, CORE, CONTEXT)
    W = len(plan)
    assert W == 9 and [int((plan[:, 0] == r).sum()) for r in range(3)] == [1, 3, 5]
    fresh, ms = plan.copy(), plan[:, 2].tolist()
    width = CORE + 2 * CONTEXT                                # the longest row: the default
    assert width == HOP * (max(ms) // HOP)
    calls = []
    kept = windows._run_windows(plan, "cpu", max_batch, max_columns, _fake(planes, calls), planes=planes)
    wide = windows._run_windows(plan.copy(), "cpu", max_batch, max_columns, _fake(planes, []), planes=planes, width=width + 3)
    assert wide.shape[:-1] == kept.shape[:-1] and wide.shape[-1] == width + 3
    assert kept.shape == ((W, width) if planes is None else (planes, W, width)) and kept.dtype == torch.float32
    # the groups are _length_groups' groups, in order, each with its contiguous rows of the plan, its samples and its range of rows
    groups = _length_groups(ms, min(max_batch, ragged.MAX_CLIPS), max_columns)
    assert [c[0] for c in calls] == groups
    if max_columns == 150:
        assert all(len(g) == 1 for g in groups if max(ms[i] for i in g) == CORE + 2 * CONTEXT) and max(len(g) for g in groups) == 2
    if max_batch <= 2:
        assert max(len(g) for g in groups) == max_batch
    done = 0
    for part, sub, m, rows in calls:
        assert sub.flags["C_CONTIGUOUS"] and np.array_equal(sub[:, :7], fresh[part][:, :7]) and np.array_equal(sub[:, 8:], fresh[part][:, 8:])
        assert m == [ms[i] for i in part] and rows == range(done, done + len(part))
        done += len(part)
    # every window's row, found through column 7, holds its own index over the columns of its group
    assert sorted(plan[:, 7].tolist()) == list(range(W))
    others = [c for c in range(plan.shape[1]) if c != 7]
    assert np.array_equal(plan[:, others], fresh[:, others])
    for part, _, m, _ in calls:
        w = HOP * (max(m) // HOP)
        for i in part:
            row = kept[..., int(plan[i, 7]), :w]
            want = float(i) if planes is None else float(i) + 1000.0 * torch.arange(planes)[:, None]
            assert bool((row == want).all()), (i, int(plan[i, 7]))
    # and all of it as the loops did it before
    before = fresh.copy()
    kept0 = _loop_before(before, max_batch, max_columns, _fake(planes, []), planes)
    assert np.array_equal(before, plan) and kept0.shape == kept.shape
    for part, _, m, rows in calls:
        w = HOP * (max(m) // HOP)
        assert torch.equal(kept0[..., rows.start:rows.stop, :w], kept[..., rows.start:rows.stop, :w])
