"""Shapes and inputs shared by tests/test_gpu_glue.py (the kernels against tests/glue_reference.py) and
tests/test_glue_reference.py (which shows, on the CPU, that these very shapes and inputs tell a wrong kernel from a right one).

The shapes are the smallest at which the kernels can go wrong; inputs are util.hashed values of O(1) magnitude, already stored
once in the mode under test (`held`: what the buffer holds, float64) -- so every term a kernel sums is exactly representable."""
import numpy as np
import torch

import glue_reference as R
from util import hashed

# (B, T, HW, C, in_cs, kt, out_cs)
STACK_CASES = [
    (2, 5, 6, 3, 16, 5, 16),        # the frames: 15 real channels + 1 padding channel, 8-channel groups straddle taps, two clips
    (2, 2, 6, 3, 16, 5, 16),        # T < kt: both sides fall outside the clip at once
    (3, 1, 4, 3, 16, 3, 16),        # T = 1
    (2, 4, 35, 24, 32, 3, 80),      # 72 real + 8 padding channels, in_cs > C
    (2, 3, 6, 64, 64, 3, 192),      # no padding
    (2, 3, 6, 16, 16, 1, 16),       # kt = 1: a copy
]
# (N, HW, C, in_cs, modes)
MEAN_CASES = [
    (6, 49, 24, 32, R.MODES),
    (4, 1, 16, 16, R.MODES),
    (3, 196, 8, 16, R.MODES),
    (2, 3136, 16, 16, ("bf16x3",)),     # in the thousands the 16-bit modes cannot see one dropped pixel
]
FEAT_ROW, FEAT_OFF = 96, 40             # the feature row the means go into / their gradients come from: per-third width, offset
CROP_B = 2
CROP_CASES = [((5, 7), (4, 9)), ((4, 9), (5, 7)), ((5, 7), (5, 7)), ((6, 8), (3, 4)), ((3, 4), (6, 8))]
FOLD_B = 2
# (H, W, pad, C, out c_off, out row)
FOLD_CASES = [
    (6, 7, 0, 16, 0, 16),           # a plain add
    (6, 7, 1, 16, 0, 16),
    (9, 11, 4, 24, 0, 32),          # the bands meet
    (5, 6, 4, 16, 0, 16),           # pad = H - 1: mirrors onto rows 0 and H - 1
    (20, 27, 2, 64, 64, 128),       # into c_off = 64 of a 128-wide buffer
]
BORDER_B = 3
BORDER_GEOMS = [(20, 27, 2, 64), (40, 37, 16, 64), (9, 11, 4, 24), (5, 6, 3, 16), (4, 7, 3, 16), (33, 18, 1, 128)]


def values(idx, shape, mode, shift=0.0):
    """float64 `shape`: hashed values (+ shift) of O(1) magnitude as a buffer of `mode` holds them after one store."""
    v = torch.from_numpy((hashed(idx, shape) + shift).astype(np.float32))
    return R.store(v, mode)


def stack_input(i, case, mode):
    B, T, HW, C = case[:4]
    return values(100 + i, (B, T, HW, C), mode)


def unstack_input(i, case, mode):
    """Gradient of the stacked tensor, non-zero in every stacked channel (padding channels included)."""
    B, T, HW, _, _, _, out_cs = case
    return values(120 + i, (B, T, HW, out_cs), mode)


def mean_input(i, case, mode):
    N, HW, C = case[:3]
    return values(140 + i, (N, HW, C), mode, shift=0.3)        # the mean is not near zero


def mean_bwd_input(i, case, mode):
    N, _, C = case[:3]
    return values(160 + i, (N, C), mode)


def crop_input(i, case, C, mode):
    (Hs, Ws), _ = case
    return values(180 + i, (CROP_B, Hs, Ws, C), mode)


def fold_inputs(i, H, W, pad, C, mode, B=FOLD_B):
    """(padded [B, H + 2 pad, W + 2 pad, C], out [B, H, W, C])."""
    return values(200 + i, (B, H + 2 * pad, W + 2 * pad, C), mode), values(220 + i, (B, H, W, C), mode)
