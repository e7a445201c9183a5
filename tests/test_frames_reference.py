"""tests/frames_reference.py checked against its own rule on the CPU: the float64 frame stitch that
tests/test_gpu_window_frames.py and tests/test_gpu_long_decisions.py hold the kernel to."""
import numpy as np
import pytest

import frames_reference as FR
import window_reference as R

HOP = 158
CORE, CONTEXT = 80 * HOP, 8 * HOP
SR = 14000
NS = [150 * HOP + 31, 3 * CORE + 5 * HOP + 77, 2 * CORE, 2 * CORE - 1, 5 * CORE + HOP - 1]
FPS = [30.0, 25.0, 29.97]


def _case(n, fps, seed=0, context=CONTEXT, F=None):
    wins = R.plan([n], CORE, CONTEXT)
    fk = FR.window_frames(wins, SR, fps, F)
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal(f).astype(np.float32) for f in fk]
    return wins, rows, FR.stitch(wins, rows, SR, fps, CORE, context, F)


def test_the_shapes_have_the_windows_zones_and_clamps_the_gpu_tests_count_on():
    assert [len(R.plan([n], CORE, CONTEXT)) for n in NS] == [1, 3, 2, 1, 5]
    for fps in FPS:
        for n in NS:
            wins, rows, st = _case(n, fps)
            assert len(st.out) == FR.n_video_frames(n, SR, fps)
            if len(wins) == 1:
                assert not st.blended.any() and st.clamped == 0
            else:
                per_zone = int(st.blended.sum()) / (len(wins) - 1)
                assert 5 <= int(st.blended.sum()) and per_zone <= 2 * CONTEXT / (SR / fps) + 1, (n, fps, int(st.blended.sum()))
    # the clamp is hit at 25 and 29.97 frames per second
    for fps in (25.0, 29.97):
        hits = [_case(n, fps)[2].clamped for n in NS]
        assert 1 <= sum(hits) and max(hits) <= 3, (fps, hits)


@pytest.mark.parametrize("fps", FPS)
@pytest.mark.parametrize("n", [NS[0], NS[3]])
def test_a_recording_of_one_window_returns_its_own_logits(n, fps):
    wins, rows, st = _case(n, fps)
    assert len(wins) == 1 and np.array_equal(st.out, rows[0].astype(np.float64)) and np.array_equal(st.index, np.arange(len(rows[0])))
    assert not st.bound.any()
    # ... and with a frame count of the caller's (a label that is not n_video_frames long)
    F = FR.n_video_frames(n, SR, fps) - 2
    wins, rows, st = _case(n, fps, F=F)
    assert len(rows[0]) == F and np.array_equal(st.out, rows[0].astype(np.float64))


@pytest.mark.parametrize("fps", FPS)
@pytest.mark.parametrize("n", NS)
def test_every_index_lies_inside_its_window_after_the_clamp(n, fps):
    wins, rows, st = _case(n, fps)
    fk = np.asarray(FR.window_frames(wins, SR, fps))
    assert np.all(st.index >= 0) and np.all(st.index < fk[st.owner])
    z = st.blended
    assert np.all(st.other_index[z] >= 0) and np.all(st.other_index[z] < fk[st.other[z]]) and np.all(np.abs(st.other[z] - st.owner[z]) == 1)
    assert np.all(st.other[~z] == -1)
    assert np.all(np.diff(st.owner) >= 0) and st.owner[0] == 0 and st.owner[-1] == len(wins) - 1


def test_the_clamp_is_hit_at_25_frames_per_second():
    """F_q is a rounded count: without the clamp a neighbour's index lands one past its last frame."""
    n = NS[4]                                                   # the five-window recording
    wins, rows, st = _case(n, 25.0)
    assert st.clamped >= 1
    fk = FR.window_frames(wins, SR, 25.0)
    rho = SR / 25.0
    past = 0
    for k, w in enumerate(wins):
        for q in (k - 1, k + 1):
            sel = (st.owner == k) & (st.other == q)
            if 0 <= q < len(wins) and sel.any():
                _, raw = FR.frame_index(np.flatnonzero(sel), wins[q].start, rho, fk[q])
                past += int((raw >= fk[q]).sum() + (raw < 0).sum())
    own_raw = [FR.frame_index(np.flatnonzero(st.owner == k), w.start, rho, fk[k])[1] for k, w in enumerate(wins)]
    past += sum(int((r >= fk[k]).sum() + (r < 0).sum()) for k, r in enumerate(own_raw))
    assert past == st.clamped
    assert any(st.other_index[i] == fk[st.other[i]] - 1 for i in np.flatnonzero(st.blended))      # ... a neighbour's last frame


@pytest.mark.parametrize("fps", FPS)
def test_context_zero_is_a_plain_cut(fps):
    n = NS[4]
    wins, rows, st = _case(n, fps, context=0)
    assert not st.blended.any() and not st.bound.any() and np.all(st.other == -1)
    want = np.array([rows[k][j] for k, j in zip(st.owner, st.index)], dtype=np.float64)
    assert np.array_equal(st.out, want)
    # outside the zones the blended stitch is the same cut
    _, _, soft = _case(n, fps)
    assert np.array_equal(soft.out[~soft.blended], st.out[~soft.blended])
    p = (np.arange(len(st.out)) + 0.5) * (SR / fps)
    assert np.array_equal(st.owner, np.minimum(np.floor(p).astype(np.int64) // CORE, len(wins) - 1))


def test_weights_are_continuous_across_a_boundary():
    """w -> 0.5 from both sides of a core boundary b: the earlier window's zone ends with it, the later one's starts with it."""
    b = 2 * CORE
    eps = np.array([1e-6, 1e-3, 0.25])
    below = FR.weight(b - eps, b - CONTEXT, CONTEXT)            # frames the earlier window owns: its upper zone
    above = FR.weight(b + eps, b - CONTEXT, CONTEXT)            # frames the later window owns: its lower zone
    assert np.all(below <= 0.5) and np.all(above >= 0.5)
    assert np.all(np.abs(below - 0.5) <= eps / (2 * CONTEXT) + 2.0 ** -24) and np.all(np.abs(above - 0.5) <= eps / (2 * CONTEXT) + 2.0 ** -24)
    assert FR.weight(np.array([b - CONTEXT]), b - CONTEXT, CONTEXT)[0] == 0.0
    assert FR.weight(np.array([b + CONTEXT - 1e-9]), b - CONTEXT, CONTEXT)[0] <= 1.0
    # in a stitch: the weights of consecutive blended frames around a boundary rise by rho / (2 context) without a jump
    wins, rows, st = _case(NS[1], 30.0)
    z = np.flatnonzero(st.blended)
    first = z[z < len(st.out) // 2]                             # the zone around the first boundary
    assert np.all(np.diff(first) == 1)
    step = (SR / 30.0) / (2 * CONTEXT)
    assert np.all(np.abs(np.diff(st.weight[first]) - step) < 1e-6)
    assert st.owner[first[0]] == 0 and st.owner[first[-1]] == 1 and 0.0 <= st.weight[first[0]] < step and 1.0 - step <= st.weight[first[-1]] < 1.0


def test_the_bound_is_four_roundings_of_the_larger_value():
    wins, rows, st = _case(NS[4], 29.97)
    z = st.blended
    own = np.array([rows[k][j] for k, j in zip(st.owner[z], st.index[z])], dtype=np.float64)
    nb = np.array([rows[k][j] for k, j in zip(st.other[z], st.other_index[z])], dtype=np.float64)
    assert np.array_equal(st.bound[z], 4.0 * 2.0 ** -24 * np.maximum(np.abs(own), np.abs(nb))) and not st.bound[~z].any()
    # an f32 blend of the same values stays inside it
    w32 = st.weight[z].astype(np.float32)
    later = st.other[z] > st.owner[z]
    a = np.where(later, own, nb).astype(np.float32)
    b = np.where(later, nb, own).astype(np.float32)
    f32 = (np.float32(1) - w32) * a + w32 * b
    assert np.all(np.abs(f32.astype(np.float64) - st.out[z]) <= st.bound[z])
