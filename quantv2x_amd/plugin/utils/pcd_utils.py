"""Point-cloud helpers of the data path; mirror of ``opencood/utils/pcd_utils.py`` (``mask_points_by_range :55-81``, ``mask_ego_points
:84-102``, ``shuffle_points :105-109``), plus two host statements of what ``IntermediateHeterFusionDataset`` does to a CAV before the model
sees it (intermediate_heter_fusion_dataset.py:129-174, :341-407): ``prepare_sweep`` -- the ego-vehicle mask and the projection in an
order-preserving form the GPU voxelizer takes as it is -- and ``select_in_range``, the communication-range selection."""
import math

import numpy as np

EGO_BOX = (-1.95, 2.95, -1.1, 1.1)                      # x_min, x_max, y_min, y_max of mask_ego_points, metres in the sensor frame


def mask_points_by_range(points, limit_range):
    """Remove the points outside ``limit_range`` = [x_min, y_min, z_min, x_max, y_max, z_max] (strict on both sides)."""
    mask = (points[:, 0] > limit_range[0]) & (points[:, 0] < limit_range[3]) & (points[:, 1] > limit_range[1]) \
        & (points[:, 1] < limit_range[4]) & (points[:, 2] > limit_range[2]) & (points[:, 2] < limit_range[5])
    return points[mask]


def _ego_hits(points):
    return (points[:, 0] >= EGO_BOX[0]) & (points[:, 0] <= EGO_BOX[1]) & (points[:, 1] >= EGO_BOX[2]) & (points[:, 1] <= EGO_BOX[3])


def mask_ego_points(points):
    """Remove the points that hit the ego vehicle itself (sensor frame).  With a float32 array numpy compares in float32 against the
    float32-rounded bounds: a point on ``float32(-1.95)`` is removed, its float32 neighbour towards minus infinity is kept."""
    return points[np.logical_not(_ego_hits(points))]


def shuffle_points(points):
    return points[np.random.permutation(points.shape[0])]


def sentinel_row():
    """(qNaN, qNaN, qNaN, 0) with the quiet NaN 0x7fc00000: what a removed point becomes in ``prepare_sweep``"""
    return np.array([0x7FC00000, 0x7FC00000, 0x7FC00000, 0], np.uint32).view(np.float32)


def prepare_sweep(points, transform=None, ego_mask=True):
    """``mask_ego_points`` then ``project_points_by_matrix_torch`` on one sweep, order-preserving: f32 [P, 4] -> f32 [P, 4] in which a point removed by
    ``mask_ego_points`` (``ego_mask``; sensor frame, before the projection), a point with a NaN coordinate and a point whose projection
    is not a number are the sentinel ``(qNaN, qNaN, qNaN, 0)``; every other point keeps its position, its intensity and -- with
    ``transform`` (4x4, rounded to float32 first) -- gets ``x' = f32(((m00 x + m01 y) + m02 z) + m03)`` in float64, ``y'``, ``z'`` alike
    (``project_points_by_matrix_torch``, box_utils.py:969-998, evaluates the same sum in float32).  The rows that are not the sentinel, in
    order, are ``mask_ego_points`` followed by the projection.  The voxelizer's key kernel gives a point with a NaN coordinate no cell
    (csrc/voxelize.hip, ``vox_keys_kernel``), so the pillars of a prepared sweep are those of the compacted one while the sweep keeps its
    length -- what a captured HIP graph needs; shorter sweeps can be padded with sentinel rows."""
    pts = np.array(points, dtype=np.float32, copy=True).reshape(-1, 4)
    drop = np.isnan(pts[:, :3]).any(axis=1)
    if ego_mask:
        drop |= _ego_hits(pts)
    if transform is not None:
        m = np.asarray(transform).astype(np.float32).astype(np.float64).reshape(4, 4)
        p = pts[:, :3].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for r in range(3):
                pts[:, r] = (((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3]).astype(np.float32)
        drop |= np.isnan(pts[:, :3]).any(axis=1)
    pts[drop] = sentinel_row()
    return pts


def kept_rows(prepared):
    """the rows of a prepared sweep that are no sentinel, in order: the compacted sweep"""
    return prepared[np.logical_not(np.isnan(prepared[:, :3]).any(axis=1))]


def select_in_range(poses, comm_range):
    """``poses`` [N, >= 2] of the candidate CAVs in ``base_data_dict`` order, the ego first -> the indices that stay, in order: candidate
    ``a`` is excluded iff ``math.sqrt(dx ** 2 + dy ** 2) > comm_range`` on the Python floats (intermediate_heter_fusion_dataset.py:343-353).
    The result is the agent layout of the scene -- host state for the voxelizer's pointer table, the engine's ``record_len`` and a
    captured graph."""
    poses = np.asarray(poses, dtype=np.float64)
    ex, ey = float(poses[0][0]), float(poses[0][1])
    return [a for a in range(poses.shape[0])
            if not math.sqrt((float(poses[a][0]) - ex) ** 2 + (float(poses[a][1]) - ey) ** 2) > comm_range]
