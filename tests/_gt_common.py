"""Shared by tests/test_gt_boxes_cpu.py and tests/test_hip_gt_boxes.py: the per-coordinate magnitude ``M`` of a projected corner, the numpy
statement run over a batch, and synthetic inputs whose every decision keeps the golden fixture's margins (no projected corner within 2e-3 m
of a range bound, no IoU within 1e-4 of the threshold) -- asserted here, rows that miss a margin are drawn again."""
from collections import OrderedDict

import numpy as np

from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gt_boxes_frame, gt_project_boxes
from quantv2x_amd.plugin.utils.eval_utils import iou_matrix

GT_RANGE = [-140.0, -40.0, -3.0, 140.0, 40.0, 1.0]
MARGIN, IOU_MARGIN, IOU_THR = 2e-3, 1e-4, 0.05


def magnitude(rows, transform, order):
    """f64 [N, 3]: per output coordinate the sum of the absolute values of the terms that form it, |T row| . (|centre| + |half extents|) +
    |translation| (the same for the 8 corners of a box)"""
    b = np.asarray(rows, np.float64)
    t = np.abs(np.asarray(transform, np.float64))
    l, w, h = (b[:, 5], b[:, 4], b[:, 3]) if order == "hwl" else (b[:, 3], b[:, 4], b[:, 5])
    cs, sn = np.abs(np.cos(b[:, 6])), np.abs(np.sin(b[:, 6]))
    local = np.stack([0.5 * l * cs + 0.5 * w * sn + np.abs(b[:, 0]), 0.5 * l * sn + 0.5 * w * cs + np.abs(b[:, 1]), 0.5 * h + np.abs(b[:, 2])], axis=1)
    return local @ t[:3, :3].T + t[:3, 3]


def statement(case):
    """the numpy statement on every frame of ``case`` -> list of dicts (``gt_boxes_frame``'s, plus ``M`` f64 [N, 3]), uncapped"""
    out = []
    for f in range(case["boxes"].shape[0]):
        n = int(np.clip(case["agent_counts"][f], 0, case["boxes"].shape[1]))
        r = gt_boxes_frame(case["boxes"][f, :n], case["mask"][f, :n], case["ids"][f, :n] if case["mode"] == 0 else None, case["transforms"][f, :n],
                           order=case["order"], mode=case["mode"], gt_range=case["gt_range"], range_xy_only=case["range_xy_only"],
                           iou_threshold=case.get("iou_threshold", IOU_THR))
        cap = case["boxes"].shape[2]
        r["M"] = np.array([magnitude(case["boxes"][f, row // cap, row % cap][None, :7], case["transforms"][f, row // cap], case["order"])[0]
                           for row in r["rows"]], np.float64).reshape(-1, 3)
        out.append(r)
    return out


def pose(g, identity=False):
    if identity:
        return np.eye(4)
    yaw, roll, pitch = g.uniform(-np.pi, np.pi), g.uniform(-0.01, 0.01), g.uniform(-0.01, 0.01)
    cz, sz, cx, sx, cy, sy = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch)
    t = np.eye(4)
    t[:3, :3] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
                 np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t[:3, 3] = [g.uniform(-20, 20), g.uniform(-10, 10), g.uniform(-0.3, 0.3)]
    return t


def ego_object(g, kind="in"):
    """x, y, z, l, w, h, yaw, label in the ego frame: firmly inside GT_RANGE ('in'), outside in y ('out'), inside in x and y only ('zout')"""
    lab = int(g.integers(1, 4))
    l, w, h = 4.2 * g.uniform(0.9, 1.1), 1.9 * g.uniform(0.9, 1.1), 1.6 * g.uniform(0.9, 1.1)
    y = g.uniform(-30, 30) if kind != "out" else g.uniform(46, 56) * g.choice([-1, 1])
    return [g.uniform(-80, 80), y, (-1.0 if kind != "zout" else 6.0) + g.uniform(-0.2, 0.2), l, w, h, g.uniform(-np.pi, np.pi), lab]


def local_row(obj, t, order, width):
    x, y, z, l, w, h, yaw, lab = obj
    p = np.linalg.inv(t) @ np.array([x, y, z, 1.0])
    dims = [h, w, l] if order == "hwl" else [l, w, h]
    return ([p[0], p[1], p[2]] + dims + [yaw - np.arctan2(t[1, 0], t[0, 0]), lab])[:width]


def _safe_row(g, kind, t, order, width, rng, obj=None):
    """the f32 row of ``obj`` (or of a fresh object of ``kind``, drawn again until it fits) under pose ``t``, its projected corners keeping
    the margin to every bound of ``rng``.  The kinds sit metres away from the bounds, so a given object's copy keeps it too: asserted."""
    bounds = np.asarray(rng, np.float64)[[0, 3, 1, 4, 2, 5]].reshape(3, 2)
    while True:
        row = np.array(local_row(obj if obj is not None else ego_object(g, kind), t, order, width), np.float32)
        c = gt_project_boxes(row[None], t.astype(np.float32), order).astype(np.float64)
        if np.abs(c[..., None] - bounds[None, None]).min() >= MARGIN:
            return row
        assert obj is None, "a shared object's copy misses the margin"


def by_id_case(seed, spec, agents, obj_cap, *, width=7, order="hwl", range_xy_only=False, used=None, id_pool=None, gt_range=GT_RANGE):
    """``spec``: per frame (survivors, duplicates, out_of_range, z_out): that many distinct in-range ids, copies of them held by other slots
    (any agent, any position: the first in (agent, slot) order is the survivor), distinct out-of-range ids and distinct ids inside in x and y
    only.  Slots not drawn stay masked and -- like every slot of an agent past ``used[f]`` -- hold in-range boxes under ids that ARE in use:
    looking at one changes the result.  ``id_pool``: the values ids are drawn from (default: any int32)."""
    g = np.random.default_rng(seed)
    F = len(spec)
    boxes = np.zeros((F, agents, obj_cap, width), np.float32); mask = np.zeros((F, agents, obj_cap), np.uint8)
    ids = np.zeros((F, agents, obj_cap), np.int32); tf = np.zeros((F, agents, 4, 4), np.float32)
    counts = np.array([agents] * F if used is None else used, np.int32)
    for f, (n_in, n_dup, n_out, n_z) in enumerate(spec):
        live = int(counts[f]) * obj_cap
        total = n_in + n_dup + n_out + n_z
        assert total <= live and (n_dup == 0 or n_in > 0)
        poses = [pose(g, a == 0) for a in range(agents)]
        tf[f] = poses
        n_ids = n_in + n_out + n_z
        if id_pool is None:
            pool = np.unique(g.integers(-2 ** 31, 2 ** 31, size=2 * n_ids + 8, dtype=np.int64))
        else:
            pool = np.asarray(id_pool, np.int64)
        own = g.choice(pool, size=n_ids, replace=False).astype(np.int32) if n_ids else np.zeros((0,), np.int32)
        objs = [(own[k], ego_object(g, "in"), "in") for k in range(n_in)]
        objs += [(own[n_in + k], None, "out") for k in range(n_out)] + [(own[n_in + n_out + k], None, "zout") for k in range(n_z)]
        objs += [objs[int(g.integers(0, n_in))] for _ in range(n_dup)]
        slots = g.permutation(live)[:total]
        for a in range(agents):
            for s in range(obj_cap):                                  # decoys first: every slot holds a plausible box under a used id
                boxes[f, a, s] = _safe_row(g, "in", poses[a], order, width, gt_range)
                ids[f, a, s] = own[int(g.integers(0, n_ids))] if n_ids else 7
        mask[f, int(counts[f]):] = 1                                  # an agent past the frame's count: mask set, still not a candidate
        for r, (oid, obj, kind) in zip(slots, objs):
            a, s = int(r) // obj_cap, int(r) % obj_cap
            row = _safe_row(g, kind, poses[a], order, width, gt_range, obj)
            boxes[f, a, s], mask[f, a, s], ids[f, a, s] = row, 1, oid
    case = {"boxes": boxes, "mask": mask, "ids": ids, "transforms": tf, "agent_counts": counts, "order": order, "mode": 0,
            "gt_range": list(gt_range), "range_xy_only": range_xy_only}
    want = statement(case)
    for f, (n_in, n_dup, n_out, n_z) in enumerate(spec):              # the inputs are what the spec says
        assert len(want[f]["rows"]) == n_in + (n_z if range_xy_only else 0), (f, len(want[f]["rows"]), spec[f])
    return case, want


def by_iou_case(seed, spec, obj_cap, *, order="hwl", used=None, gt_range=GT_RANGE):
    """``spec``: per frame (vehicle boxes, infrastructure boxes overlapping exactly one vehicle box, infrastructure boxes overlapping none).
    Objects sit in the cells of a 10 m x 5 m grid (a box's half diagonal is below 2.5 m: two cells never overlap); an overlapping box shares
    its vehicle box's cell, 0.3 m to the side."""
    g = np.random.default_rng(seed)
    F = len(spec)
    boxes = np.zeros((F, 2, obj_cap, 7), np.float32); mask = np.zeros((F, 2, obj_cap), np.uint8); tf = np.zeros((F, 2, 4, 4), np.float32)
    counts = np.array([2] * F if used is None else used, np.int32)
    cells = [(x, y) for x in np.arange(-75, 80, 10.0) for y in np.arange(-27.5, 30, 5.0)]
    for f, (n_veh, n_hit, n_free) in enumerate(spec):
        poses = [pose(g, a == 0) for a in range(2)]
        tf[f] = poses
        order_cells = g.permutation(len(cells))
        assert n_veh + n_free <= len(cells) and n_hit <= n_veh and max(n_veh, n_hit + n_free) <= obj_cap
        veh = []
        for k in range(n_veh):
            o = ego_object(g, "in")
            o[0], o[1] = cells[order_cells[k]]
            veh.append(o)
        inf = []
        for k in range(n_hit):
            o = list(veh[k])
            o[0] += -np.sin(o[6]) * 0.3; o[1] += np.cos(o[6]) * 0.3
            inf.append(o)
        for k in range(n_free):
            o = ego_object(g, "in")
            o[0], o[1] = cells[order_cells[n_veh + k]]
            inf.append(o)
        inf = [inf[i] for i in g.permutation(len(inf))]
        for a, objs in enumerate([veh, inf]):
            for s in range(obj_cap):
                boxes[f, a, s] = local_row(veh[int(g.integers(0, n_veh))] if n_veh else ego_object(g, "in"), poses[a], order, 7)   # decoys ON vehicle boxes
            for s, o in zip(np.sort(g.permutation(obj_cap)[:len(objs)]), objs):
                boxes[f, a, s], mask[f, a, s] = local_row(o, poses[a], order, 7), 1
    case = {"boxes": boxes, "mask": mask, "ids": None, "transforms": tf, "agent_counts": counts, "order": order, "mode": 1,
            "gt_range": list(gt_range), "range_xy_only": True, "iou_threshold": IOU_THR}
    bounds = np.asarray(gt_range, np.float64)[[0, 3, 1, 4]].reshape(2, 2)
    for f in range(F):                                                # the margins, on what the statement itself projects
        n = int(counts[f])
        c = [gt_project_boxes(boxes[f, a][mask[f, a] == 1], tf[f, a], order).astype(np.float64) for a in range(n)]
        for q in c:
            assert q.size == 0 or np.abs(q[..., :2, None] - bounds[None, None]).min() >= MARGIN
        if n == 2:
            iou = iou_matrix(c[1][:, :4, :2], c[0][:, :4, :2])
            assert iou.size == 0 or np.abs(iou - np.float32(IOU_THR)).min() >= IOU_MARGIN
    want = statement(case)
    for f, (n_veh, n_hit, n_free) in enumerate(spec):
        assert len(want[f]["rows"]) == (n_veh + n_free if counts[f] == 2 else n_veh), (f, len(want[f]["rows"]), spec[f])
    return case, want


def data_dicts(case, transform_key, as_torch=True):
    """the reference-shaped per-frame ``data_dict``s of a case: an OrderedDict of cav_content per frame"""
    import torch
    conv = (lambda v: torch.from_numpy(np.ascontiguousarray(v))) if as_torch else (lambda v: np.array(v))
    out = []
    for f in range(case["boxes"].shape[0]):
        d = OrderedDict()
        for a in range(int(case["agent_counts"][f])):
            m = case["mask"][f, a] == 1
            d[f"cav{a}"] = {"object_bbx_center": conv(case["boxes"][f, a]), "object_bbx_mask": conv(case["mask"][f, a].astype(np.float32)),
                            "object_ids": [int(v) for v in case["ids"][f, a][m]] if case["ids"] is not None else [],
                            transform_key: conv(case["transforms"][f, a])}
        out.append(d)
    return out


def golden_case(fx, which):
    """tests/golden/gt_boxes.npz as a case: 'single', 'mc' or 'iou'"""
    if which == "iou":
        return {"boxes": fx["iou_boxes"], "mask": fx["iou_mask"], "ids": None, "transforms": fx["iou_transforms"], "agent_counts": fx["iou_agent_counts"],
                "order": str(fx["order"]), "mode": 1, "gt_range": fx["gt_range"].tolist(), "range_xy_only": True, "iou_threshold": IOU_THR}
    single = which == "single"
    return {"boxes": np.ascontiguousarray(fx["boxes"][..., :7]) if single else fx["boxes"], "mask": fx["mask"], "ids": fx["ids"],
            "transforms": fx["transforms"], "agent_counts": fx["agent_counts"], "order": str(fx["order"]), "mode": 0,
            "gt_range": (fx["gt_range"] if single else fx["gt_range_mc"]).tolist(), "range_xy_only": not single}
