"""tests/golden/scene_prep.npz: the reference's own, unmodified scene-preparation functions on synthetic inputs -- data only.

* ``x_to_world``, ``x1_to_x2`` and ``get_pairwise_transformation`` (opencood/utils/transformation_utils.py:264-334, :21-66) on ten scenes of
  1 to 5 CAVs (each count twice), ``max_cav`` 5, ``proj_first`` both ways.  Yaw covers the full circle (the scenes' first agents sit at
  -180, -90, 0, 90 and 180 degrees exactly), roll and pitch are non-zero, positions reach 1000 m; the agents of a scene lie within 120 m of
  their ego.  ``ref_to_ego[s, a] = x1_to_x2(pose a, pose 0)``, the call of intermediate_heter_fusion_dataset.py:131-134.
* ``mask_ego_points`` (opencood/utils/pcd_utils.py:84-102) and ``project_points_by_matrix_torch`` (opencood/utils/box_utils.py:969-998) on
  four sweeps.  A sweep holds random points (a third of them around the ego box) and, for each of the four bounds of the ego box rounded
  to float32, three points with the other coordinate well inside the box: one exactly on the bound, one a float32 step inside, one a
  step outside.  The intensity column holds the row index (exact in float32), so the rows the reference kept are read off its output:
  ``ref_kept``.  ``ref_projected`` is the reference's float32 projection of the kept rows by ``sweep_transforms`` (an ``x1_to_x2`` result,
  handed over in float64 as the dataset does).
* the in-range decision of intermediate_heter_fusion_dataset.py:343-353.  It is inline in ``__getitem__``, so ``in_range`` below RESTATES
  that one expression (``math.sqrt(dx ** 2 + dy ** 2) > comm_range`` on the pose lists' Python floats); nothing else here is restated.
  Six candidate lists; besides random agents each holds deliberate ones about 1e-9 m inside and beyond the range, and one list an agent
  at exactly the range from an ego at the origin (kept: the comparison is strict).

The script asserts its own margins: no pose distance lies within 1e-6 m of ``comm_range`` other than the deliberate ones, and those lie
within 1e-8 m of it on the intended side; every random sweep point is at least 1e-3 m from every bound of the ego box.

Run in the build container only (the reference tree is imported through ``_refimport``): ``python tests/golden/make_golden_scene.py``."""
import math
import os
import sys
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(os.path.dirname(HERE))]
import _refimport  # noqa: E402

MAX_CAV, SCENE_COUNTS, COMM_RANGE, SEED = 5, [1, 2, 3, 4, 5, 5, 4, 3, 2, 1], 70.0, 20260
EGO_YAWS = [-180.0, -90.0, 0.0, 90.0, 180.0]
BOUNDS = [(0, -1.95, -1), (0, 2.95, 1), (1, -1.1, -1), (1, 1.1, 1)]        # (axis, bound, the direction that leaves the box)


def in_range(pose, ego_pose, comm_range):
    """RESTATED from intermediate_heter_fusion_dataset.py:343-353 (inline there): the agent is excluded iff distance > comm_range"""
    distance = math.sqrt((pose[0] - ego_pose[0]) ** 2 + (pose[1] - ego_pose[1]) ** 2)
    return not distance > comm_range


def random_pose(g, centre=None):
    if centre is None:
        x, y = g.uniform(-1000, 1000), g.uniform(-1000, 1000)
    else:
        r, th = g.uniform(3, 120), g.uniform(0, 2 * np.pi)
        x, y = centre[0] + r * np.cos(th), centre[1] + r * np.sin(th)
    return [float(x), float(y), float(g.uniform(-5, 5)), float(g.uniform(-6, 6)), float(g.uniform(-180, 180)), float(g.uniform(-6, 6))]


def scene_part(g, tu):
    S = len(SCENE_COUNTS)
    poses = np.zeros((S, MAX_CAV, 6))
    world = np.tile(np.eye(4), (S, MAX_CAV, 1, 1))
    to_ego = np.tile(np.eye(4), (S, MAX_CAV, 1, 1))
    pair = np.zeros((S, MAX_CAV, MAX_CAV, 4, 4))
    pair_proj = np.zeros_like(pair)
    for s, n in enumerate(SCENE_COUNTS):
        ego = random_pose(g)
        if s < len(EGO_YAWS):
            ego[4] = EGO_YAWS[s]
        if s == 0:
            ego[0], ego[1] = 1000.0, -1000.0
        lst = [ego] + [random_pose(g, ego) for _ in range(n - 1)]
        base = OrderedDict((str(a), {"params": {"lidar_pose": list(p)}}) for a, p in enumerate(lst))
        for a, p in enumerate(lst):
            poses[s, a] = p
            world[s, a] = tu.x_to_world(list(p))
            to_ego[s, a] = tu.x1_to_x2(list(p), list(ego))
        pair[s] = tu.get_pairwise_transformation(base, MAX_CAV, False)
        pair_proj[s] = tu.get_pairwise_transformation(base, MAX_CAV, True)
    assert np.abs(poses[..., :2]).max() == 1000.0 and (poses[:, :, [3, 5]][poses[:, :, 4] != 0] != 0).all()
    return {"poses": poses, "counts": np.array(SCENE_COUNTS, np.int32), "ref_world": world, "ref_to_ego": to_ego, "ref_pairwise": pair,
            "ref_pairwise_proj": pair_proj}


def sweep(g, n_random):
    far = np.stack([g.uniform(-60, 60, n_random), g.uniform(-40, 40, n_random)], 1)
    near = np.stack([g.uniform(-4, 5, n_random // 2), g.uniform(-2.5, 2.5, n_random // 2)], 1)
    xy = np.concatenate([far, near]).astype(np.float32)
    ok = np.ones(len(xy), bool)
    for axis, b, _ in BOUNDS:                                                   # the random points keep clear of the bounds
        ok &= np.abs(xy[:, axis].astype(np.float64) - b) >= 1e-3
    xy = xy[ok]
    edge = []
    for axis, b, out in BOUNDS:
        b32 = np.float32(b)
        other = np.float32(0.4 if axis == 0 else 0.7)
        for v in (b32, np.nextafter(b32, np.float32(-out * np.inf)), np.nextafter(b32, np.float32(out * np.inf))):
            edge.append([v, other] if axis == 0 else [other, v])
    xy = np.concatenate([xy, np.array(edge, np.float32)])
    xy = xy[g.permutation(len(xy))]
    pts = np.zeros((len(xy), 4), np.float32)
    pts[:, :2], pts[:, 2] = xy, g.uniform(-3, 1, len(xy)).astype(np.float32)
    pts[:, 3] = np.arange(len(xy), dtype=np.float32)                           # the row index: which rows the reference kept
    return pts


def sweep_part(g, tu, pcd_utils, box_utils):
    out, sizes = {}, [700, 900, 500, 800]
    P = max(sizes) * 2
    pts_all = np.zeros((len(sizes), P, 4), np.float32)
    n_all = np.zeros(len(sizes), np.int32)
    kept_all = np.zeros((len(sizes), P), bool)
    proj_all = np.zeros((len(sizes), P, 3), np.float32)
    tf_all = np.zeros((len(sizes), 4, 4))
    for k, n_random in enumerate(sizes):
        pts = sweep(g, n_random)
        ego = random_pose(g)
        tf = tu.x1_to_x2(random_pose(g, ego), ego)
        masked = pcd_utils.mask_ego_points(pts.copy())
        rows = masked[:, 3].astype(np.int64)
        assert (pts[rows] == masked).all() and (np.diff(rows) > 0).all()
        projected = box_utils.project_points_by_matrix_torch(masked[:, :3], tf)
        assert projected.dtype == np.float32 and projected.shape == (len(rows), 3)
        n = len(pts)
        pts_all[k, :n], n_all[k], tf_all[k] = pts, n, tf
        kept_all[k, rows] = True
        proj_all[k, :len(rows)] = projected
    out.update({"sweeps": pts_all, "sweep_points": n_all, "sweep_transforms": tf_all, "ref_kept": kept_all, "ref_projected": proj_all})
    return out


def range_part(g):
    G, N = 6, 8
    poses, counts, kept = np.zeros((G, N, 6)), np.zeros(G, np.int32), np.zeros((G, N), bool)
    deliberate = np.zeros((G, N), bool)
    for k in range(G):
        ego = random_pose(g)
        if k == 0:
            ego[0], ego[1] = 0.0, 0.0
        lst, marks = [ego], [False]
        for _ in range(int(g.integers(2, 5))):
            r, th = g.uniform(5, 140), g.uniform(0, 2 * np.pi)
            p = random_pose(g)
            p[0], p[1] = ego[0] + r * np.cos(th), ego[1] + r * np.sin(th)
            lst.append(p); marks.append(False)
        for delta in (-1e-9, 1e-9):                                           # just inside, just beyond
            th = g.uniform(0, 2 * np.pi)
            p = random_pose(g)
            p[0], p[1] = ego[0] + (COMM_RANGE + delta) * np.cos(th), ego[1] + (COMM_RANGE + delta) * np.sin(th)
            d = math.sqrt((p[0] - ego[0]) ** 2 + (p[1] - ego[1]) ** 2)
            assert 0 < (d - COMM_RANGE) * np.sign(delta) < 1e-8, (k, delta, d)
            lst.append(p); marks.append(True)
        if k == 0:                                                             # exactly at the range: kept
            p = random_pose(g)
            p[0], p[1] = COMM_RANGE, 0.0
            assert math.sqrt((p[0] - ego[0]) ** 2 + (p[1] - ego[1]) ** 2) == COMM_RANGE
            lst.append(p); marks.append(True)
        order = [0] + [int(i) + 1 for i in g.permutation(len(lst) - 1)]
        lst, marks = [lst[i] for i in order], [marks[i] for i in order]
        for a, p in enumerate(lst):
            d = math.sqrt((p[0] - ego[0]) ** 2 + (p[1] - ego[1]) ** 2)
            assert marks[a] or abs(d - COMM_RANGE) > 1e-6, (k, a, d)
            poses[k, a], kept[k, a], deliberate[k, a] = p, in_range(p, ego, COMM_RANGE), marks[a]
        counts[k] = len(lst)
    assert kept[:, 0].all() and kept[deliberate].sum() == G + 1 and (~kept[deliberate]).sum() == G
    return {"range_poses": poses, "range_counts": counts, "comm_range": np.float64(COMM_RANGE), "ref_in_range": kept, "range_deliberate": deliberate}


def main():
    _refimport.install()
    ov = types.ModuleType("opencood.utils.box_overlaps")                       # a compiled extension the package imports for training labels
    ov.bbox_overlaps = lambda *a, **k: None
    sys.modules.setdefault("opencood.utils.box_overlaps", ov)
    from opencood.utils import box_utils, pcd_utils
    from opencood.utils import transformation_utils as tu
    g = np.random.default_rng(SEED)
    out = {"seed": np.int64(SEED), "max_cav": np.int32(MAX_CAV)}
    out.update(scene_part(g, tu))
    out.update(sweep_part(g, tu, pcd_utils, box_utils))
    out.update(range_part(g))
    path = os.path.join(HERE, "scene_prep.npz")
    np.savez_compressed(path, **out)
    print("scenes", out["counts"].tolist(), "| sweep points", out["sweep_points"].tolist(), "kept", out["ref_kept"].sum(1).tolist(),
          "| range", out["range_counts"].tolist(), "kept", out["ref_in_range"].sum(1).tolist(), "|", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
