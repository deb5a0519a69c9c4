"""``VoxelPostprocessor`` of ``opencood/data_utils/post_processor/voxel_postprocessor.py`` for inference: same
constructor, ``generate_anchor_box`` (:30-83) and ``post_process(data_dict, output_dict)`` (:245-405) contract, the
work done by ``qv2x_postprocess_f32`` (``csrc/postprocess.hip``).  Training-side members (``generate_label``,
``collate_batch``, ``visualize``) are out of scope (datasets / training).

``post_process`` handles what intermediate / early fusion produces (``output_dict`` with the ego entry only) and late fusion (one
entry per CAV: ``qv2x_postprocess_late_f32``, up to 8 CAVs).  The head maps must live on the GPU (they come from ``DeployedModel``);
there is no CPU fallback.

``generate_gt_bbx`` (base_postprocessor.py:47-107) and ``generate_gt_bbx_by_iou`` (:110-200) run ``qv2x_gt_boxes_f32`` (``csrc/gt_boxes.hip``)
as a batch of one and read back, because the reference's callers expect a sized tensor; ``quantv2x_amd.ground_truth`` is the batched surface
that reads nothing back.  ``gt_boxes_frame`` below is the numpy statement of that entry's contract (include/qv2x.h), the way
``eval_utils.tp_fp_frame`` states the evaluator's: fp64 with one rounding, the CPU and GPU tests compare against it.
"""
import ctypes as C
import math

import numpy as np
import torch

from ....lib import PostprocessDesc, check, current_stream, load, ptr


def load_point_pillar_anchor_args(hypes: dict) -> dict:
    """``yaml_utils.load_point_pillar_params`` (hypes_yaml/yaml_utils.py:106-146), the post-process part: fills
    ``vw, vh, vd, W, H, D`` of ``hypes['postprocess']['anchor_args']`` from the lidar range and the voxel size."""
    r = hypes["preprocess"]["cav_lidar_range"]
    vw, vh, vd = hypes["preprocess"]["args"]["voxel_size"]
    a = hypes["postprocess"]["anchor_args"]
    a.update(vw=vw, vh=vh, vd=vd, W=math.ceil((r[3] - r[0]) / vw), H=math.ceil((r[4] - r[1]) / vh), D=math.ceil((r[5] - r[2]) / vd))
    return hypes


def _desc(owner, maps, *, anchors_per_cell, num_classes, num_bins, dir_offset, rng, range_xy_only, max_extent, z_lim, max_boxes) -> PostprocessDesc:
    """the descriptor of a call on head maps ``[N, C, H, W]`` (``transform`` left to the caller: only the single-CAV C entry reads it)"""
    d = PostprocessDesc()
    d.h, d.w, d.anchors_per_cell, d.num_bins = int(maps.shape[2]), int(maps.shape[3]), anchors_per_cell, num_bins
    d.score_threshold = float(owner.params["target_args"]["score_threshold"])
    d.nms_threshold = float(owner.params["nms_thresh"])
    d.dir_offset = dir_offset
    for i, v in enumerate(rng):
        d.range[i] = float(v)
    d.max_boxes, d.num_classes, d.range_xy_only = max_boxes, num_classes, int(range_xy_only)
    d.max_extent, d.z_min, d.z_max = max_extent, z_lim[0], z_lim[1]
    return d


def _workspace(owner, need: int, dev, query: str):
    """``owner``'s workspace, kept between frames and grown to ``need`` bytes on ``dev`` (a negative ``need`` is ``query``'s refusal)"""
    if need < 0:
        check(-1, query)
    if owner._ws is None or owner._ws.numel() < need or owner._ws.device != dev:
        owner._ws = torch.empty(need, dtype=torch.uint8, device=dev)
    return ptr(owner._ws)


def gpu_post_process(owner, cls, reg, dirp, anchors_dev, transformation_matrix, *, anchors_per_cell, num_classes, num_bins, dir_offset,
                     rng, range_xy_only, max_extent, z_lim, max_boxes, sync=True):
    """One ``qv2x_postprocess_f32`` call (or, when ``cls`` / ``reg`` / ``dirp`` / ``anchors_dev`` / ``transformation_matrix`` are lists with
    one entry per CAV, one ``qv2x_postprocess_late_f32`` call); ``owner`` keeps the workspace between frames.
    -> (corners [K, 8, 3], scores [K], labels i32 [K]) on the GPU, or (None, None, None)."""
    lib = load()
    many = isinstance(cls, (list, tuple))
    cls_l, reg_l = (list(cls), list(reg)) if many else ([cls], [reg])
    dir_l = (list(dirp) if many else [dirp]) if dirp is not None else [None] * len(cls_l)
    anc_l = list(anchors_dev) if many else [anchors_dev]
    t_l = list(transformation_matrix) if many else [transformation_matrix]
    ncav = len(cls_l)
    dev = cls_l[0].device
    d = _desc(owner, cls_l[0], anchors_per_cell=anchors_per_cell, num_classes=num_classes, num_bins=num_bins, dir_offset=dir_offset,
              rng=rng, range_xy_only=range_xy_only, max_extent=max_extent, z_lim=z_lim, max_boxes=max_boxes)
    tf = (C.c_float * (16 * ncav))()
    for c, t in enumerate(t_l):
        t = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float32).reshape(16)
        for i in range(16):
            tf[c * 16 + i] = float(t[i])
            if c == 0:
                d.transform[i] = float(t[i])
    need = lib.qv2x_postprocess_late_workspace_bytes(C.byref(d), ncav)
    ws = _workspace(owner, need, dev, "qv2x_postprocess_late_workspace_bytes")
    corners = torch.empty((max_boxes, 8, 3), dtype=torch.float32, device=dev)
    scores = torch.empty((max_boxes,), dtype=torch.float32, device=dev)
    labels = torch.empty((max_boxes,), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    f32 = lambda x: x.to(torch.float32).contiguous()
    cls_l, reg_l = [f32(x) for x in cls_l], [f32(x) for x in reg_l]
    dir_l = [f32(x) if (x is not None and num_bins > 0) else None for x in dir_l]
    arr = lambda ts: (C.c_void_p * ncav)(*[(t.data_ptr() if t is not None else None) for t in ts])
    check(lib.qv2x_postprocess_late_f32(C.byref(d), ncav, arr(cls_l), arr(reg_l), arr(dir_l), arr(anc_l), tf, ws, need,
                                        ptr(corners), ptr(scores), ptr(labels), ptr(count), current_stream()), "qv2x_postprocess_late_f32")
    if not sync:                                     # HIP-graph capture: fixed-size outputs + the box count left on the device
        return corners, scores, labels, count
    k = int(count.item())                            # the one host synchronisation of the frame (the reference goes to numpy here)
    if k == 0:
        return None, None, None
    return corners[:k], scores[:k], labels[:k]


def _frame_maps(x, frames):
    """f32 head maps [frames, C, H, W] with every frame's [C, H, W] block dense (the frames themselves may lie at any stride: a slice of a
    larger tensor is taken as it is) -> (tensor, floats between two frames)"""
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.shape[0] != frames:
        raise ValueError(f"head maps {tuple(x.shape)}: {frames} frames expected")
    c, h, w = (int(v) for v in x.shape[1:])
    if tuple(x.stride()[1:]) != (h * w, w, 1) or (frames > 1 and x.stride(0) < c * h * w):
        x = x.contiguous()
    return x, (int(x.stride(0)) if frames > 1 else c * h * w)


def gpu_post_process_batch(owner, cls, reg, dirp, anchors_dev, transformation_matrix, *, anchors_per_cell, num_classes, num_bins, dir_offset,
                           rng, range_xy_only, max_extent, z_lim, max_boxes):
    """``frames`` independent frames in ONE ``qv2x_postprocess_batch_f32`` call: ``cls`` / ``reg`` / ``dirp`` are ``[frames, C, H, W]`` head
    maps (``dirp`` None without a direction head), ``anchors_dev`` the shared anchors, ``transformation_matrix`` a ``[frames, 4, 4]`` tensor
    (taken as it is when it already is a contiguous f32 tensor on the maps' device -- what a HIP-graph capture needs: nothing is copied
    from the host).  Nothing is read back: -> (corners [frames, max_boxes, 8, 3], scores [frames, max_boxes], labels i32
    [frames, max_boxes], counts i32 [frames]) on the GPU; frame ``f``'s boxes are the first ``counts[f]`` rows of ``corners[f]``, bit for bit
    what ``gpu_post_process`` returns for that frame."""
    lib = load()
    frames, dev = int(cls.shape[0]), cls.device
    d = _desc(owner, cls, anchors_per_cell=anchors_per_cell, num_classes=num_classes, num_bins=num_bins, dir_offset=dir_offset,
              rng=rng, range_xy_only=range_xy_only, max_extent=max_extent, z_lim=z_lim, max_boxes=max_boxes)
    t = torch.as_tensor(transformation_matrix)
    if tuple(t.shape) != (frames, 4, 4):
        raise ValueError(f"transformation_matrix {tuple(t.shape)}: ({frames}, 4, 4) expected")
    if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=dev, dtype=torch.float32).contiguous()
    need = lib.qv2x_postprocess_batch_workspace_bytes(C.byref(d), frames)
    ws = _workspace(owner, need, dev, "qv2x_postprocess_batch_workspace_bytes")
    corners = torch.empty((frames, max_boxes, 8, 3), dtype=torch.float32, device=dev)
    scores = torch.empty((frames, max_boxes), dtype=torch.float32, device=dev)
    labels = torch.empty((frames, max_boxes), dtype=torch.int32, device=dev)
    counts = torch.zeros((frames,), dtype=torch.int32, device=dev)
    cls, cs = _frame_maps(cls, frames)
    reg, rs = _frame_maps(reg, frames)
    dirp, ds = _frame_maps(dirp, frames) if (dirp is not None and num_bins > 0) else (None, 0)
    check(lib.qv2x_postprocess_batch_f32(C.byref(d), frames, ptr(cls), cs, ptr(reg), rs, ptr(dirp), ds, ptr(anchors_dev), ptr(t),
                                         ws, need, ptr(corners), ptr(scores), ptr(labels), ptr(counts), current_stream()),
          "qv2x_postprocess_batch_f32")
    return corners, scores, labels, counts


# ---- ground truth: the numpy statement of qv2x_gt_boxes_f32 -----------------------------------------------------------------------------
_TEMPLATE = np.array([[1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, -1], [1, -1, 1], [1, 1, 1], [-1, 1, 1], [-1, -1, 1]], np.float64)
GT_ORDERS = {"hwl": 0, "lwh": 1}


def gt_project_boxes(rows, transform, order):
    """f32 box rows [N, >= 7] (``order`` 'hwl': x, y, z, h, w, l, yaw; 'lwh': x, y, z, l, w, h, yaw) and a 4x4 transform -> f32 [N, 8, 3]:
    ``boxes_to_corners_3d`` + ``project_box3d`` (box_utils.py:152-204, :278-316) from the f32 inputs in float64, rounded once; the sums in
    the order include/qv2x.h states."""
    b = np.asarray(rows, np.float32).astype(np.float64).reshape(-1, np.shape(rows)[-1])
    t = np.asarray(transform, np.float32).astype(np.float64)
    lwh = b[:, [5, 4, 3]] if GT_ORDERS[order] == 0 else b[:, 3:6]
    p = (0.5 * lwh)[:, None, :] * _TEMPLATE[None]                   # [N, 8, 3]
    cs, sn = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    x = (p[..., 0] * cs - p[..., 1] * sn) + b[:, None, 0]
    y = (p[..., 0] * sn + p[..., 1] * cs) + b[:, None, 1]
    z = p[..., 2] + b[:, None, 2]
    return np.stack([((t[i, 0] * x + t[i, 1] * y) + t[i, 2] * z) + t[i, 3] for i in range(3)], axis=-1).astype(np.float32)


def gt_boxes_frame(boxes, mask, ids, transforms, *, order, mode, gt_range, range_xy_only, iou_threshold=0.05):
    """One frame of ``qv2x_gt_boxes_f32`` in numpy.  ``boxes`` f32 [agents, obj_cap, 7 or 8], ``mask`` [agents, obj_cap], ``ids`` i32
    [agents, obj_cap] (None in mode 1), ``transforms`` [agents, 4, 4]: the agents in use only.  Candidates are the rows with their mask set, in
    (agent, slot) order; mode 0 keeps a candidate iff no earlier candidate has its id, mode 1 keeps agent 0's and those of agent 1 whose
    ``float32(inter / union)`` with every candidate of agent 0 is ``<= float32(iou_threshold)`` (bottom faces of the projected f32 boxes,
    ``eval_utils.iou_matrix``); then the survivor's own f32 corners are range-masked (``>=`` / ``<=`` against the f32 bounds, all 8 corners,
    x and y or x, y and z).  -> dict: ``corners`` f32 [N, 8, 3], ``labels`` i32 [N] (None for 7-float rows), ``ids`` i32 [N] (mode 1: the row
    agent * obj_cap + slot), ``rows`` i64 [N], in candidate order, uncapped."""
    from ...utils.eval_utils import iou_matrix
    boxes = np.asarray(boxes, np.float32)
    agents, cap, width = boxes.shape
    if mode == 1 and agents > 2:
        raise ValueError("mode 1 takes at most 2 agents")
    cand = np.nonzero(np.asarray(mask).reshape(-1) != 0)[0]           # rows agent * obj_cap + slot, ascending
    if agents == 0 or cand.size == 0:
        corners = np.zeros((0, 8, 3), np.float32)
    else:
        corners = np.concatenate([gt_project_boxes(boxes[a][cand[cand // cap == a] % cap], np.asarray(transforms)[a], order) for a in range(agents)])
    if mode == 0:
        flat = np.asarray(ids, np.int32).reshape(-1)[cand]
        seen, keep = set(), np.zeros((cand.size,), bool)
        for k, v in enumerate(flat.tolist()):
            keep[k] = v not in seen
            seen.add(v)
    else:
        first = cand // cap == 0
        keep = first.copy()
        q = corners[:, :4, :2].astype(np.float64)
        iou = iou_matrix(q[~first], q[first])
        keep[~first] = ~(iou > np.float32(iou_threshold)).any(axis=1)
        flat = cand.astype(np.int32)
    rng = np.asarray(gt_range, np.float32)
    dims = 2 if range_xy_only else 3
    inside = ((corners[..., :dims] >= rng[:dims]) & (corners[..., :dims] <= rng[3:3 + dims])).all(axis=(1, 2))
    keep &= inside
    return {"corners": corners[keep], "labels": boxes.reshape(-1, width)[cand[keep], 7].astype(np.int32) if width == 8 else None,
            "ids": flat[keep].astype(np.int32), "rows": cand[keep]}


def _gt_from_data_dict(owner, data_dict, by_iou=False):
    """the reference-named methods: one frame through ``quantv2x_amd.ground_truth`` on the GPU, read back to a sized result
    -> (corners [N, 8, 3], labels i32 [N] or None)"""
    from ....ground_truth import MAX_GT, MAX_OBJ, GroundTruthAssembler
    n = max(1, len(data_dict))
    cap = min(MAX_OBJ, max([1] + [int(np.shape(c["object_bbx_center"])[0]) for c in data_dict.values()]))
    key = (n, cap, by_iou)
    if getattr(owner, "_gt_asm", None) is None or owner._gt_asm[0] != key:
        owner._gt_asm = (key, GroundTruthAssembler(owner, max_agents=n, obj_cap=cap, gt_cap=MAX_GT, frames=1, by_iou=by_iou))
    out = owner._gt_asm[1].fill([data_dict])()
    count, total = (int(v) for v in torch.stack([out["counts"][0], out["totals"][0]]).tolist())    # the one host synchronisation (the reference goes to numpy here)
    if total > count:
        raise RuntimeError(f"{total} ground-truth boxes in one frame: the evaluator's layout holds {count}")
    return out["corners"][0, :count].clone(), (out["labels"][0, :count].clone() if out["labels"] is not None else None)


class VoxelPostprocessor:
    def __init__(self, anchor_params, train):
        self.params = anchor_params
        self.train = train
        self.bbx_dict = {}
        self.anchor_num = self.params["anchor_args"]["num"]
        self._ws = None
        self._anchors_dev = None

    def generate_anchor_box(self):
        a = self.params["anchor_args"]
        r = [math.radians(e) for e in a["r"]]
        assert self.anchor_num == len(r)
        stride = a.get("feature_stride", 2)
        lr = a["cav_lidar_range"]
        x = np.linspace(lr[0] + a["vw"], lr[3] - a["vw"], a["W"] // stride)
        y = np.linspace(lr[1] + a["vh"], lr[4] - a["vh"], a["H"] // stride)
        cx, cy = np.meshgrid(x, y)
        cx = np.tile(cx[..., np.newaxis], self.anchor_num)
        cy = np.tile(cy[..., np.newaxis], self.anchor_num)
        cz = np.ones_like(cx) * -1.0
        w, l, h = np.ones_like(cx) * a["w"], np.ones_like(cx) * a["l"], np.ones_like(cx) * a["h"]
        r_ = np.ones_like(cx)
        for i in range(self.anchor_num):
            r_[..., i] = r[i]
        if self.params["order"] == "hwl":
            return np.stack([cx, cy, cz, h, w, l, r_], axis=-1)
        if self.params["order"] == "lhw":
            return np.stack([cx, cy, cz, l, h, w, r_], axis=-1)
        raise SystemExit("Unknown bbx order.")

    # ---- inference -------------------------------------------------------------------------------------------
    def post_process(self, data_dict, output_dict, max_boxes: int = 1000):
        """-> (pred_box3d_tensor [K, 8, 3], scores [K]) on the GPU, or (None, None) when nothing passes."""
        if self.params["order"] != "hwl":
            raise NotImplementedError("deployed post-process: box order 'hwl' (PointPillar)")
        cavs = [c for c in data_dict if c in output_dict]              # late fusion: one entry per CAV, the reference's loop order
        if not 1 <= len(cavs) <= 8:
            raise NotImplementedError("deployed post-process: 1..8 CAVs per call")
        cls_l, reg_l, dir_l, anc_l, t_l = [], [], [], [], []
        for cav_id in cavs:
            out, cav = output_dict[cav_id], data_dict[cav_id]
            cls = out["cls_preds"] if "cls_preds" in out else out["psm"]
            reg = out["reg_preds"] if "reg_preds" in out else out["rm"]
            dirp = out.get("dir_preds", out.get("dm"))
            if not cls.is_cuda:
                raise RuntimeError("VoxelPostprocessor.post_process runs on the GPU (libqv2x): the head maps must be CUDA tensors")
            if cls.shape[0] != 1 or cls.shape[1] != self.anchor_num:
                raise ValueError(f"cls_preds {tuple(cls.shape)}: batch 1 and {self.anchor_num} anchors per cell expected")
            h, w = int(cls.shape[2]), int(cls.shape[3])
            anchors = cav["anchor_box"]
            # device copies by anchor OBJECT (late fusion: every CAV carries its own `anchor_box`; one slot keyed on identity missed on
            # every CAV of every frame and re-uploaded H*W*A*7 floats each time); the entry keeps the object alive, so its id is not reused
            hit = self._anchors_dev.get(id(anchors)) if self._anchors_dev else None
            if hit is None or hit[0] is not anchors:
                a32 = torch.as_tensor(np.asarray(anchors.cpu() if torch.is_tensor(anchors) else anchors)).to(torch.float32)
                if tuple(a32.shape) != (h, w, self.anchor_num, 7):
                    raise ValueError(f"anchor_box {tuple(a32.shape)} does not match the head maps ({h}, {w}, {self.anchor_num}, 7)")
                if self._anchors_dev is None or len(self._anchors_dev) >= 16:
                    self._anchors_dev = {}
                hit = self._anchors_dev[id(anchors)] = (anchors, a32.reshape(-1, 7).contiguous().to(cls.device))
            cls_l.append(cls); reg_l.append(reg); dir_l.append(dirp); anc_l.append(hit[1]); t_l.append(cav["transformation_matrix"])
        has_dir = all(x is not None for x in dir_l)
        boxes, scores, _ = gpu_post_process(
            self, cls_l, reg_l, dir_l if has_dir else None, anc_l, t_l, anchors_per_cell=self.anchor_num,
            num_classes=1, num_bins=int(self.params["dir_args"]["num_bins"]) if has_dir else 0,
            dir_offset=float(self.params["dir_args"]["dir_offset"]) if has_dir else 0.0,
            rng=self.params["gt_range"], range_xy_only=False, max_extent=6.0, z_lim=(-3.0, 1.0), max_boxes=max_boxes)
        return boxes, scores

    # ---- ground truth ----------------------------------------------------------------------------------------
    def generate_gt_bbx(self, data_dict):
        """-> gt_box3d_tensor [N, 8, 3] on the GPU: the CAVs' boxes projected with ``transformation_matrix_clean``, de-duplicated by object
        id (first occurrence, in that order: the reference's order is a ``set()``'s) and masked to ``gt_range`` on x, y and z."""
        return _gt_from_data_dict(self, data_dict)[0]

    def generate_gt_bbx_by_iou(self, data_dict):
        """-> gt_box3d_tensor [N, 8, 3] on the GPU (DAIR-V2X late fusion: two label sources, no ids): the second source's boxes whose BEV IoU
        with a box of the first exceeds 0.05 are dropped, then the mask to ``gt_range`` on x and y."""
        if len(data_dict) > 2:
            raise NotImplementedError("generate_gt_bbx_by_iou: one or two label sources")
        return _gt_from_data_dict(self, data_dict, by_iou=True)[0]
