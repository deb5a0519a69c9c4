"""The grid and depth-bin helpers of the reference's camera branch under its names (opencood/utils/camera_utils.py:129-135, 187-196):
what ``LiftSplatShoot.__init__`` and ``create_frustum`` call, and ``bin_depths`` (:137-185) of the ground-truth depth path.  Results are bit-equal to
the reference's (tests/golden/lift_splat.npz, tests/golden/cam_encode.npz)."""
import math

import numpy as np
import torch


def gen_dx_bx(xbound, ybound, zbound):
    """``[low, high, step]`` per axis -> (dx f32 [3] cell size, bx f32 [3] centre of the first cell, nx i64 [3] cells).  The Python
    doubles are rounded to float32 once; the cell count is the double quotient truncated toward zero, as ``torch.LongTensor`` does."""
    bounds = (xbound, ybound, zbound)
    dx = torch.tensor([float(b[2]) for b in bounds], dtype=torch.float32)
    bx = torch.tensor([b[0] + b[2] / 2.0 for b in bounds], dtype=torch.float32)
    nx = torch.tensor([int((b[1] - b[0]) / b[2]) for b in bounds], dtype=torch.int64)
    return dx, bx, nx


def depth_discretization(depth_min, depth_max, num_bins, mode):
    """The lower edges of ``num_bins`` depth bins, float64 [num_bins]: ``UD`` uniform, ``LID`` linearly increasing bin sizes
    (https://arxiv.org/abs/2005.13423)."""
    k = np.arange(num_bins)
    if mode == "UD":
        bin_size = (depth_max - depth_min) / num_bins
        return depth_min + bin_size * k
    if mode == "LID":
        bin_size = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
        return depth_min + bin_size * (k * np.arange(1, 1 + num_bins)) / 2
    raise NotImplementedError(f"depth discretization mode {mode!r}: 'UD' or 'LID'")


def bin_depths(depth_map, mode, depth_min, depth_max, num_bins, target=True):
    """Metric depth -> depth-bin index, int64, the inverse of ``depth_discretization`` (plus ``SID``, log-spaced bins; reference
    camera_utils.py:137-185).  The fractional index is clamped into ``[0, num_bins - 1]``, NaN and +inf landing in the last bin and -inf in
    the first.  ``target=True`` (training targets) returns ``(indices, None)``; ``target=False`` also returns the mask of the depths that
    lay INSIDE the range before the clamp, which ``get_gt_depth_dist`` multiplies onto the one-hot."""
    if mode == "UD":
        step = (depth_max - depth_min) / num_bins
        frac = (depth_map - depth_min) / step
    elif mode == "LID":
        step = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
        frac = -0.5 + 0.5 * torch.sqrt(1 + 8 * (depth_map - depth_min) / step)
    elif mode == "SID":
        frac = num_bins * (torch.log(1 + depth_map) - math.log(1 + depth_min)) / (math.log(1 + depth_max) - math.log(1 + depth_min))
    else:
        raise NotImplementedError(f"depth discretization mode {mode!r}: 'UD', 'LID' or 'SID'")
    outside = (frac < 0) | (frac >= num_bins) | ~torch.isfinite(frac)
    last = torch.full_like(frac, num_bins - 1)
    frac = torch.where(frac < 0, torch.zeros_like(frac), frac)
    frac = torch.where(frac >= num_bins, last, frac)
    frac = torch.where(torch.isfinite(frac), frac, last)
    return frac.type(torch.int64), (None if target else ~outside)
