"""tests/golden/eval.npz: the reference's own, unmodified evaluator -- ``opencood/utils/eval_utils.py`` (``caluclate_tp_fp :40-120`` over 3
thresholds x 4 ranges, ``calculate_ap :124-166``) and ``opencood/utils/eval_utils_mc.py`` (``caluclate_tp_fp :41-93`` per class,
``calculate_ap :95-133``) -- on six synthetic frames of at most 60 detections and 40 GT: GT boxes jittered in position, yaw and size (IoUs
spread over [0, 1]), near-duplicates that compete for one GT, clutter, labels 1..3.  Detections are stored in descending score order per
frame, the way every post-processor delivers them.

What this pins is the evaluator's CONTROL FLOW: range filter, score order, greedy matching with removal, the AP arithmetic.  It does NOT
pin shapely's areas: shapely is absent here and un-vendored, so the reference runs with a minimal ``Polygon`` stand-in in the stubbed
``shapely.geometry`` that offers ``centroid.x`` / ``centroid.y`` (the four corners summed in index order times 0.25), ``intersection(b).area``
and ``union(b).area`` on top of ``oracle.postprocess.quad_intersection_area`` / ``quad_area`` -- the same position as the rotated NMS, whose
polygon IoU is unpinned in exactly this way (oracle/postprocess.py).

The script asserts about its own inputs, reseeding until all hold (the seed is stored): all scores of the fixture are distinct, so the
reference's unstable sorts cannot matter; no IoU lies within 1e-4 of a threshold; no centre distance lies within 1e-3 m of a range bound.

Run in the build container only (the reference tree is imported through ``_refimport``): ``python tests/golden/make_golden_eval.py``."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(os.path.dirname(HERE))]
import _refimport  # noqa: E402

THRESHOLDS = (0.3, 0.5, 0.7)
RANGES = ((-float("inf"), float("inf")), (0.0, 30.0), (30.0, 50.0), (50.0, 100.0))
FRAMES, DET_CAP, GT_CAP, CLASSES = 6, 60, 40, 3


class _Area:
    def __init__(self, area):
        self.area = area


class _Point:
    def __init__(self, x, y):
        self.x, self.y = x, y


class Polygon:
    """what eval_utils / common_utils use of shapely's Polygon, for convex quadrilaterals"""

    def __init__(self, pts):
        self.q = [(float(x), float(y)) for x, y in pts]
        assert len(self.q) == 4

    @property
    def centroid(self):
        q = self.q
        return _Point((q[0][0] + q[1][0] + q[2][0] + q[3][0]) * 0.25, (q[0][1] + q[1][1] + q[2][1] + q[3][1]) * 0.25)

    def intersection(self, other):
        from oracle.postprocess import quad_intersection_area
        return _Area(quad_intersection_area(self.q, other.q))

    def union(self, other):
        from oracle.postprocess import quad_area, quad_intersection_area
        return _Area(quad_area(self.q) + quad_area(other.q) - quad_intersection_area(self.q, other.q))


def corners(x, y, l, w, yaw):
    """f32 [8, 3]: bottom face first, the corner order of box_utils.boxes_to_corners_3d"""
    t = np.array([[1, -1], [1, 1], [-1, 1], [-1, -1]], np.float64) * 0.5 * np.array([l, w])
    c, s = np.cos(yaw), np.sin(yaw)
    xy = np.stack([t[:, 0] * c - t[:, 1] * s + x, t[:, 0] * s + t[:, 1] * c + y], axis=1)
    out = np.zeros((8, 3), np.float32)
    out[:4, :2] = out[4:, :2] = xy
    out[:4, 2], out[4:, 2] = -1.0, 0.6
    return out


def scene(seed):
    g = np.random.default_rng(seed)
    det = np.zeros((FRAMES, DET_CAP, 8, 3), np.float32); dsc = np.zeros((FRAMES, DET_CAP), np.float32)
    dlab = np.zeros((FRAMES, DET_CAP), np.int32); dn = np.zeros((FRAMES,), np.int32)
    gt = np.zeros((FRAMES, GT_CAP, 8, 3), np.float32); glab = np.zeros((FRAMES, GT_CAP), np.int32); gn = np.zeros((FRAMES,), np.int32)
    for f in range(FRAMES):
        n_gt = int(g.integers(18, GT_CAP + 1)) if f else GT_CAP
        boxes, rows = [], []
        for k in range(n_gt):
            if k and g.random() < 0.25:                              # parked next to the previous one
                px, py, pl, pw, pyaw, plab = boxes[-1]
                x, y, yaw, lab = px - np.sin(pyaw) * (pw + 0.5), py + np.cos(pyaw) * (pw + 0.5), pyaw, plab
            else:
                r, a = g.uniform(3.0, 108.0), g.uniform(-np.pi, np.pi)
                x, y, yaw, lab = r * np.cos(a), r * np.sin(a), g.uniform(-np.pi, np.pi), int(g.integers(1, CLASSES + 1))
            l, w = [(4.2, 1.9), (0.8, 0.7), (9.0, 2.6)][lab - 1]
            l, w = l * g.uniform(0.85, 1.15), w * g.uniform(0.85, 1.15)
            boxes.append((x, y, l, w, yaw, lab))
            gt[f, k], glab[f, k] = corners(x, y, l, w, yaw), lab
        gn[f] = n_gt
        for k, (x, y, l, w, yaw, lab) in enumerate(boxes):
            if g.random() < 0.12:
                continue                                              # missed
            j = g.uniform(0.0, 1.0) ** 2                              # jitter strength: most detections sit well, some barely overlap
            copies = 2 if g.random() < 0.3 else 1                     # near-duplicates competing for this GT
            for c in range(copies):
                jj = j if c == 0 else min(1.0, j + g.uniform(0.02, 0.3))
                rows.append((corners(x + g.normal(0, 0.9 * l * 0.5) * jj, y + g.normal(0, 0.9 * w) * jj, l * (1 + g.uniform(-0.3, 0.3) * jj),
                                     w * (1 + g.uniform(-0.3, 0.3) * jj), yaw + g.normal(0, 0.5) * jj),
                             float(np.clip(g.uniform(0.35, 0.99) - 0.25 * jj, 0.05, 0.999)), lab if g.random() < 0.9 else int(g.integers(1, CLASSES + 1))))
        while len(rows) < DET_CAP and (g.random() < 0.9 or f == 1):   # clutter (frame 1 is filled to the cap)
            r, a, lab = g.uniform(3.0, 108.0), g.uniform(-np.pi, np.pi), int(g.integers(1, CLASSES + 1))
            l, w = [(4.2, 1.9), (0.8, 0.7), (9.0, 2.6)][lab - 1]
            rows.append((corners(r * np.cos(a), r * np.sin(a), l, w, g.uniform(-np.pi, np.pi)), float(g.uniform(0.05, 0.6)), lab))
        rows = rows[:DET_CAP]
        rows.sort(key=lambda e: -np.float32(e[1]))
        dn[f] = len(rows)
        for k, (c, s, lab) in enumerate(rows):
            det[f, k], dsc[f, k], dlab[f, k] = c, s, lab
    return det, dsc, dlab, dn, gt, glab, gn


def margins_hold(det, dsc, dn, gt, gn):
    from oracle.postprocess import quad_area, quad_intersection_area
    sc = np.concatenate([dsc[f, :dn[f]] for f in range(FRAMES)])
    if len(np.unique(sc)) != len(sc):
        return False
    bounds = np.array([b for r in RANGES for b in r if np.isfinite(b)])
    for f in range(FRAMES):
        for q in list(det[f, :dn[f]]) + list(gt[f, :gn[f]]):
            p = Polygon(q[:4, :2]).centroid
            if np.abs(np.sqrt(p.x ** 2 + p.y ** 2) - bounds).min() < 1e-3:
                return False
        for a in det[f, :dn[f]]:
            for b in gt[f, :gn[f]]:
                qa, qb = a[:4, :2].astype(np.float64), b[:4, :2].astype(np.float64)
                inter = quad_intersection_area(qa, qb)
                union = quad_area(qa) + quad_area(qb) - inter
                if not union > 0 or np.abs(np.float32(inter / union) - np.array(THRESHOLDS)).min() < 1e-4:
                    return False
    return True


def main():
    import torch
    _refimport.install()
    sys.modules["shapely.geometry"].Polygon = Polygon
    from opencood.utils import eval_utils, eval_utils_mc
    seed = 20240
    while True:
        det, dsc, dlab, dn, gt, glab, gn = scene(seed)
        if margins_hold(det, dsc, dn, gt, gn):
            break
        seed += 1
    out = {"seed": np.int64(seed), "thresholds": np.array(THRESHOLDS, np.float64), "ranges": np.array(RANGES, np.float64),
           "det_corners": det, "det_scores": dsc, "det_labels": dlab, "det_counts": dn, "gt_corners": gt, "gt_labels": glab, "gt_counts": gn}
    # class-agnostic, per range: eval_utils
    for ri, (left, right) in enumerate(RANGES):
        stat = {t: {"tp": [], "fp": [], "gt": 0, "score": []} for t in THRESHOLDS}
        for f in range(FRAMES):
            for t in THRESHOLDS:
                eval_utils.caluclate_tp_fp(torch.from_numpy(det[f, :dn[f]]), torch.from_numpy(dsc[f, :dn[f]]), torch.from_numpy(gt[f, :gn[f]]),
                                           stat, t, left, right)
        for ti, t in enumerate(THRESHOLDS):
            k = f"r{ri}_t{ti}"
            out["tp_" + k], out["fp_" + k] = np.array(stat[t]["tp"], np.uint8), np.array(stat[t]["fp"], np.uint8)
            out["score_" + k], out["gt_" + k] = np.array(stat[t]["score"], np.float32), np.int64(stat[t]["gt"])
            ap, mrec, mpre = eval_utils.calculate_ap(stat, t)
            out["ap_" + k], out["mrec_" + k], out["mpre_" + k] = np.float64(ap), np.array(mrec, np.float64), np.array(mpre, np.float64)
    # per class, no range: eval_utils_mc (the multi-class tools hand over one class's boxes per call, None when it has no detection)
    for c in range(1, CLASSES + 1):
        stat = {t: {"tp": [], "fp": [], "gt": 0} for t in THRESHOLDS}
        for f in range(FRAMES):
            dm, gm = dlab[f, :dn[f]] == c, glab[f, :gn[f]] == c
            for t in THRESHOLDS:
                db = torch.from_numpy(det[f, :dn[f]][dm]) if dm.any() else None
                eval_utils_mc.caluclate_tp_fp(db, torch.from_numpy(dsc[f, :dn[f]][dm]), torch.from_numpy(gt[f, :gn[f]][gm]), stat, t)
        for ti, t in enumerate(THRESHOLDS):
            k = f"c{c}_t{ti}"
            out["mc_tp_" + k], out["mc_fp_" + k] = np.array(stat[t]["tp"], np.uint8), np.array(stat[t]["fp"], np.uint8)
            out["mc_gt_" + k] = np.int64(stat[t]["gt"])
            ap, mrec, mpre = eval_utils_mc.calculate_ap(copy.deepcopy(stat), t)
            out["mc_ap_" + k], out["mc_mrec_" + k], out["mc_mpre_" + k] = np.float64(ap), np.array(mrec, np.float64), np.array(mpre, np.float64)
    path = os.path.join(HERE, "eval.npz")
    np.savez_compressed(path, **out)
    print("seed", seed, "detections", dn.tolist(), "gt", gn.tolist(), os.path.getsize(path), "bytes")
    for ri in range(len(RANGES)):
        print("range", ri, ["%.4f" % out[f"ap_r{ri}_t{ti}"] for ti in range(3)], "gt", int(out[f"gt_r{ri}_t0"]),
              "tp", [int(out[f"tp_r{ri}_t{ti}"].sum()) for ti in range(3)])
    for c in range(1, CLASSES + 1):
        print("class", c, ["%.4f" % out[f"mc_ap_c{c}_t{ti}"] for ti in range(3)], "gt", int(out[f"mc_gt_c{c}_t0"]))


if __name__ == "__main__":
    main()
