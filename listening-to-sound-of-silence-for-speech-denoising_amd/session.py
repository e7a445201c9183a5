"""What the streaming sessions share (stream.StreamDenoiser, stream_resampling.StreamResampler, stream_resampling.StreamBandMerger): a fixed number of slots, each holding an
open stream or None, chunks of any size per slot, and a device ring per slot filled by sos_stream_push_f32."""
import numpy as np
import torch

from . import _lib as L


def open_slots(who, slots, streams):
    """close / drop: `slots` (one, or an iterable) as a list; each holds an open stream (streams[slot] is not None), none twice."""
    slots = [slots] if isinstance(slots, int) else list(slots)
    for s in slots:
        if not isinstance(s, int) or not 0 <= s < len(streams) or streams[s] is None:
            raise ValueError(f"{who}: slot {s!r} has no open stream")
    if len(set(slots)) != len(slots):
        raise ValueError(f"{who}: a slot is named twice")
    return slots


def check_chunks(who, chunks, n_slots):
    for s, c in chunks.items():
        if not isinstance(s, int) or not 0 <= s < n_slots:
            raise ValueError(f"{who}: unknown slot {s!r} (0 .. {n_slots - 1})")
        if not (torch.is_tensor(c) or isinstance(c, np.ndarray)) or c.ndim != 1 or c.dtype != (torch.float32 if torch.is_tensor(c) else np.float32):
            raise ValueError(f"{who}: slot {s}: a chunk is a 1-D float32 GPU tensor or numpy array")
        if torch.is_tensor(c):
            L.require_cuda(c)


def empty(device):
    return torch.empty(0, dtype=torch.float32, device=device)


def fill_rounds(slots, offs, left, state):
    """A chunk larger than its free ring goes in pieces: yields, while samples are left, the rows {slot, source offset, samples,
    stream position} of one sos_stream_push_f32 launch, every slot taking what fits.  offs, left: where each slot's chunk goes on
    in the flat buffer and how much is left (advanced here); state(slot) -> (free samples of its ring, position of its next
    sample), asked anew every round: the caller accounts for a round's rows before the next."""
    while any(left):
        rows = []
        for i, s in enumerate(slots):
            free, position = state(s)
            take = min(left[i], free)
            if take:
                rows.append((s, offs[i], take, position))
                offs[i], left[i] = offs[i] + take, left[i] - take
        yield rows
