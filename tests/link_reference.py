"""numpy restatement of what sos_window_frames_link_f32 (csrc/ragged_window.hip) adds to the frame stitch: the reduction of the
stitched logits over the recordings of a link group, and the decision.  Independent of the package; the stitch itself is
tests/frames_reference.py's.  Everything is float32 in the kernel's operation order, so the kernel's logits are compared bit
for bit.  The decision goes through an exponential, which numpy and the device round differently in the last place: sigmoid()
returns the float64 value next to it, so that a test can tell the frames where that matters."""
import numpy as np

MODES = ("any", "mean")


def link(logits_per_member, mode):
    """One float32 stream out of the members' streams (equal lengths), reduced IN MEMBER ORDER.  'any': the running maximum
    (fmaxf); 'mean': a sequential float32 sum, then one float32 divide by the member count."""
    rows = [np.ascontiguousarray(m, dtype=np.float32) for m in logits_per_member]
    if not rows or any(r.shape != rows[0].shape for r in rows) or mode not in MODES:
        raise ValueError("link: one or more members of one shape, mode 'any' or 'mean'")
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = np.fmax(acc, r) if mode == "any" else (acc + r).astype(np.float32)
    if mode == "mean":
        acc = (acc / np.float32(len(rows))).astype(np.float32)
    return acc


def sigmoid(x):
    """(float32 1 / (1 + exp(-x)) in float32 steps, the same in float64)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        s32 = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x).astype(np.float32))).astype(np.float32)
        s64 = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    return s32, s64


def decide(x, thr=0.5):
    """uint8 decisions, 1 = non-silent: 1 / (1 + exp(-x)) >= thr, every step in float32."""
    return (sigmoid(x)[0] >= np.float32(thr)).astype(np.uint8)


def near_threshold(x, thr=0.5):
    """Frames whose float64 sigmoid lies within float32 rounding of the threshold: three operations (exp, add, divide) of half
    an ulp each, plus the exponential's own few ulps on either side -- 8 * 2^-24 relative.  Only there may two correct float32
    evaluations of the decision differ."""
    s64 = sigmoid(x)[1]
    return np.abs(s64 - float(np.float32(thr))) <= 8.0 * 2.0 ** -24 * np.maximum(s64, float(np.float32(thr)))


def tables(ids, frames):
    """The link tables out of one group id per recording (None: a group of its own) and the recordings' frame counts.  Groups
    in the order of their first member, members in recording order.
    -> (links int64 (groups, 4) = {frame offset of the group's stream, frames, first index into members, member count},
    members int64, group of each recording int64)."""
    groups, where = [], {}
    for r, g in enumerate(ids):
        if g is None:
            groups.append([r])
        elif g in where:
            groups[where[g]].append(r)
        else:
            where[g] = len(groups)
            groups.append([r])
    links, members, foff = [], [], 0
    for m in groups:
        links.append((foff, int(frames[m[0]]), len(members), len(m)))
        foff += int(frames[m[0]])
        members += m
    group = np.zeros(len(ids), dtype=np.int64)
    for g, m in enumerate(groups):
        group[m] = g
    return np.asarray(links, dtype=np.int64).reshape(-1, 4), np.asarray(members, dtype=np.int64), group
