"""The ragged layer of the package (csrc/ragged.h is its other half): clips of any lengths back to back in one buffer plus a
table of where each lies.  Package-internal; nothing here touches the GPU at import."""
import numpy as np
import torch

from . import _lib as L

MAX_CLIPS = 65535                   # clips per launch sequence (the kernels' grid.y); every chunking loop reads it when called


def offsets(lens):
    """Where each of consecutive spans of `lens` elements starts: int64 cumsum(lens) - lens."""
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    return np.cumsum(lens, dtype=np.int64) - lens


def clip_table(ns, nb=None):
    """Host int64 [B][4] rows {sample offset, samples, frame offset, frames} of clips of ns samples and nb (default 0) frames."""
    tab = np.zeros((len(ns), 4), dtype=np.int64)
    tab[:, 1] = ns
    if nb is not None:
        tab[:, 3] = nb
    np.cumsum(tab[:-1, 1::2], axis=0, out=tab[1:, 0::2])              # both offset columns: one call (one-clip tables are hot)
    return tab


def chunks(n):
    """The spans (c0, c1) of a launch sequence over n clips: consecutive, of at most MAX_CLIPS clips each."""
    for c0 in range(0, n, MAX_CLIPS):
        yield c0, min(c0 + MAX_CLIPS, n)


def host_table(rows, cols=None):
    """The host copy of a launch table: integers, given as rows of `cols` entries or (cols=None) as stacked rows or columns
    whose shape stays, -> a C-contiguous int64 array.  An empty table is refused."""
    tab = np.asarray(rows, dtype=np.int64)
    tab = np.ascontiguousarray(tab if cols is None else tab.reshape(-1, cols))
    if tab.size < 1:
        raise ValueError("an empty table")
    return tab


def upload(host, device):
    """The device copy of a host table (int64) or of a per-clip array (float64): engine.upload, which does not wait for the
    stream."""
    from .engine import upload as staged                         # when called: engine is not loaded for the host-only users
    return staged(host, torch.int64 if host.dtype == np.int64 else torch.float64, device)


def table(rows, device, cols=None):
    """Both copies of a launch table: (host_table(rows, cols), its upload)."""
    tab = host_table(rows, cols)
    return tab, upload(tab, device)


def back_to_back(tensors):
    """One 1-D tensor holding the elements of `tensors` in order: a view when they already lie back to back in one buffer (what
    ragged.split, resample_batch_device and denoise_long return), their concatenation otherwise."""
    first = tensors[0]
    at, base = first.storage_offset(), first.untyped_storage().data_ptr()
    for t in tensors:
        if not t.is_contiguous() or t.untyped_storage().data_ptr() != base or t.storage_offset() != at or t.dtype != first.dtype:
            return torch.cat([t.reshape(-1) for t in tensors])
        at += t.numel()
    return first.as_strided((at - first.storage_offset(),), (1,), first.storage_offset())


def flat_f32(tensors, device):
    """back_to_back of 1-D f32 tensors of which some (or all) may be empty: never a null pointer."""
    full = [t for t in tensors if t.numel()]
    return back_to_back(full) if full else torch.zeros(1, dtype=torch.float32, device=device)


def group_by(keys, skip=None):
    """{key: the indices that have it, ascending}, keys in order of first appearance, without the indices i for which
    skip(i, keys[i])."""
    groups = {}
    for i, key in enumerate(keys):
        if skip is None or not skip(i, key):
            groups.setdefault(key, []).append(i)
    return groups


def per_group(items, keys, run, skip=None):
    """One batch call per key: a copy of `items` in which items[i], for every index i of every group of group_by(keys, skip), is
    replaced by the i-th result of run(key, indices of the group) -- one result per index, in order."""
    out = list(items)
    for key, idx in group_by(keys, skip).items():
        for i, y in zip(idx, run(key, idx)):
            out[i] = y
    return out


def per_clip(value, nclips, name):
    """A scalar or one value per clip -> a writable f64 array of `nclips` values."""
    v = np.asarray(value, dtype=np.float64)
    if v.ndim > 1 or (v.ndim == 1 and len(v) != nclips):
        raise ValueError(f"{name}: one value or one per clip ({nclips}), got shape {v.shape}")
    return np.array(np.broadcast_to(v, (nclips,)))


def device_f32(x):
    """A signal (numpy array or GPU tensor) as a contiguous 1-D f32 GPU tensor."""
    if not torch.cuda.is_available():
        raise RuntimeError("sos_amd.metrics needs an MI355X: there is no CPU fallback")
    if torch.is_tensor(x):
        L.require_cuda(x)
        return x.detach().reshape(-1).float().contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.float32)).cuda()


def concat(signals):
    """One f32 device buffer holding the signals back to back (plus a zero sentinel, so that it is never empty), and
    their lengths.  numpy inputs go up in one copy; tensors must live on the GPU."""
    if not any(torch.is_tensor(s) for s in signals):
        flat = [np.asarray(s, dtype=np.float32).reshape(-1) for s in signals]
        return device_f32(np.concatenate(flat + [np.zeros(1, np.float32)])), [len(f) for f in flat]
    ts = [device_f32(s) for s in signals]
    return torch.cat(ts + [torch.zeros(1, dtype=torch.float32, device=ts[0].device)]), [t.numel() for t in ts]


def split(flat, lens):
    """Views of consecutive spans of `lens` elements of a 1-D tensor or array."""
    return [flat[o:o + n] for o, n in zip(offsets(lens).tolist(), np.asarray(lens, dtype=np.int64).reshape(-1).tolist())]


def byte_groups(sizes, max_bytes):
    """Consecutive indices 0 .. len(sizes) in groups of at most max_bytes (an entry larger than that is a group of its own) and
    at most MAX_CLIPS entries."""
    groups, cur, size = [], [], 0
    for i, nb in enumerate(sizes):
        if cur and (size + nb > max_bytes or len(cur) >= MAX_CLIPS):
            groups.append(cur)
            cur, size = [], 0
        cur.append(i)
        size += nb
    if cur:
        groups.append(cur)
    return groups


def download(tensors, dtype=None):
    """The 1-D GPU tensors of a list as host arrays (of `dtype`, if given), through one copy of their concatenation."""
    if not tensors:
        return []
    flat = np.ascontiguousarray((torch.cat(tensors) if len(tensors) > 1 else tensors[0]).cpu().numpy(), dtype=dtype)
    return split(flat, [t.numel() for t in tensors])
