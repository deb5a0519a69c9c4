"""Ground-truth boxes on the device: ``qv2x_gt_boxes_f32`` behind a thin wrapper, and an assembler that turns the reference's per-frame
``data_dict``s into what ``DetectionEvaluator.update`` takes -- the CAVs' object lists projected into the ego frame, de-duplicated and
range-masked (``generate_gt_bbx`` / ``generate_gt_bbx_by_iou`` of opencood/data_utils/post_processor) -- without a device-to-host copy."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .lib import GtDesc, check, current_stream, load, ptr

MAX_FRAMES, MAX_AGENTS, MAX_OBJ, MAX_GT = 64, 8, 256, 256
ORDERS = {"hwl": 0, "lwh": 1}


def _dev_tensor(t, dtype, dev, shape, name):
    t = torch.as_tensor(t)
    if t.device != dev or t.dtype != dtype or not t.is_contiguous():
        t = t.to(device=dev, dtype=dtype, non_blocking=True).contiguous()
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} {tuple(t.shape)}: {shape} expected")
    return t


def gpu_gt_boxes_batch(boxes, mask, ids, transforms, agent_counts, *, order, mode, gt_range, range_xy_only, gt_cap, iou_threshold=0.05, out=None):
    """``qv2x_gt_boxes_f32`` on a batch (include/qv2x.h has the conventions).  ``boxes`` f32 [frames, agents, obj_cap, 7 or 8], ``mask`` u8
    [frames, agents, obj_cap], ``ids`` i32 [frames, agents, obj_cap] (None in mode 1), ``transforms`` f32 [frames, agents, 4, 4], ``agent_counts``
    i32 [frames], all on one GPU; ``order`` 'hwl' or 'lwh', ``mode`` 0 (by id) or 1 (by IoU).  Range bounds and the threshold are rounded to
    float32.  Nothing is read back and nothing waits: -> dict ``corners`` f32 [frames, gt_cap, 8, 3], ``labels`` i32 [frames, gt_cap] (None
    for 7-float rows), ``ids`` i32 [frames, gt_cap], ``counts`` / ``totals`` i32 [frames] on the GPU; ``totals[f] > counts[f]`` says that frame
    ``f`` had more than ``gt_cap`` boxes.  Rows past ``counts[f]`` keep what the buffers held (zeros when they are allocated here; ``out``, a
    dict of that form, is written in place).  More than 64 frames go in calls of 64."""
    lib = load()
    dev = boxes.device
    if dev.type != "cuda":
        raise ValueError("gpu_gt_boxes_batch: tensors on the GPU expected (the CPU statement is plugin...voxel_postprocessor.gt_boxes_frame)")
    if boxes.dim() != 4:
        raise ValueError(f"boxes {tuple(boxes.shape)}: [frames, agents, obj_cap, 7 or 8] expected")
    frames, agents, cap, width = (int(v) for v in boxes.shape)
    if order not in ORDERS:
        raise ValueError(f"order {order!r}: 'hwl' or 'lwh'")
    boxes = _dev_tensor(boxes, torch.float32, dev, (frames, agents, cap, width), "boxes")
    mask = _dev_tensor(mask, torch.uint8, dev, (frames, agents, cap), "mask")
    ids = _dev_tensor(ids, torch.int32, dev, (frames, agents, cap), "ids") if (ids is not None and mode == 0) else None
    transforms = _dev_tensor(transforms, torch.float32, dev, (frames, agents, 4, 4), "transforms")
    agent_counts = _dev_tensor(agent_counts, torch.int32, dev, (frames,), "agent_counts")
    if out is None:
        out = {"corners": torch.zeros((frames, gt_cap, 8, 3), dtype=torch.float32, device=dev),
               "labels": torch.zeros((frames, gt_cap), dtype=torch.int32, device=dev) if width == 8 else None,
               "ids": torch.zeros((frames, gt_cap), dtype=torch.int32, device=dev),
               "counts": torch.zeros((frames,), dtype=torch.int32, device=dev), "totals": torch.zeros((frames,), dtype=torch.int32, device=dev)}
    else:
        for k, dt, shape in (("corners", torch.float32, (frames, gt_cap, 8, 3)), ("labels", torch.int32, (frames, gt_cap)),
                             ("ids", torch.int32, (frames, gt_cap)), ("counts", torch.int32, (frames,)), ("totals", torch.int32, (frames,))):
            t = out.get(k)
            if t is None and k == "labels" and width == 7:
                continue
            if t is None or t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out[{k!r}]: a contiguous {dt} tensor {shape} on {dev} expected")
    d = GtDesc()
    d.agents, d.obj_cap, d.gt_cap, d.row_floats, d.order, d.mode = agents, cap, int(gt_cap), width, ORDERS[order], int(mode)
    d.range_xy_only, d.iou_threshold = int(bool(range_xy_only)), float(iou_threshold)
    for i, v in enumerate(gt_range):
        d.range[i] = float(v)
    stream = current_stream()
    for f0 in range(0, max(frames, 1), MAX_FRAMES):
        f1 = min(frames, f0 + MAX_FRAMES)
        d.frames = f1 - f0
        part = lambda t: ptr(t[f0:f1]) if t is not None else ptr(None)      # noqa: E731  (a slice of the leading dimension: contiguous)
        check(lib.qv2x_gt_boxes_f32(C.byref(d), part(boxes), part(mask), part(ids), part(transforms), part(agent_counts), part(out["corners"]),
                                    part(out["labels"] if width == 8 else None), part(out["ids"]), part(out["counts"]), part(out["totals"]),
                                    stream), "qv2x_gt_boxes_f32")
    return out


class GroundTruthAssembler:
    """Fixed device buffers for ``frames`` frames of up to ``max_agents`` CAVs with ``obj_cap`` object rows each; ``fill`` writes them in place
    from the reference's per-frame ``data_dict``s, a call enqueues ``qv2x_gt_boxes_f32`` on them and returns the (equally fixed) output
    dict of ``gpu_gt_boxes_batch`` -- so a call can be captured in a HIP graph and replayed after every ``fill``.

    What is read and how follows the post-processor: ``VoxelPostprocessor`` -- 7-float rows, ``transformation_matrix_clean``, the range mask
    of ``params['gt_range']`` on x, y and z (``generate_gt_bbx``) or, with ``by_iou``, the IoU filter of two label sources and the mask on
    x and y (``generate_gt_bbx_by_iou``); ``VoxelPostprocessor3Heads`` -- 8-float rows with the label last, ``transformation_matrix``,
    ``GT_RANGE`` on x and y."""

    def __init__(self, postprocessor, max_agents, obj_cap, gt_cap, frames=1, by_iou=False, device="cuda"):
        from .plugin.data_utils.post_processor.voxel_postprocessor_3heads import VoxelPostprocessor3Heads
        multi = isinstance(postprocessor, VoxelPostprocessor3Heads)
        if multi and by_iou:
            raise ValueError("by_iou: the single-class post-processor only")
        if not (1 <= max_agents <= (2 if by_iou else MAX_AGENTS) and 1 <= obj_cap <= MAX_OBJ and 1 <= gt_cap <= MAX_GT and frames >= 1):
            raise ValueError(f"max_agents in 1..{2 if by_iou else MAX_AGENTS}, obj_cap in 1..{MAX_OBJ}, gt_cap in 1..{MAX_GT}, frames >= 1")
        self.order = postprocessor.order if multi else postprocessor.params["order"]
        if self.order not in ORDERS:
            raise ValueError(f"box order {self.order!r}: 'hwl' or 'lwh'")
        self.mode, self.row_floats = (1 if by_iou else 0), (8 if multi else 7)
        self.transform_key = "transformation_matrix" if multi else "transformation_matrix_clean"
        self.gt_range = [float(v) for v in (postprocessor.gt_range if multi else postprocessor.params["gt_range"])]
        self.range_xy_only = bool(multi or by_iou)
        self.frames, self.max_agents, self.obj_cap, self.gt_cap = int(frames), int(max_agents), int(obj_cap), int(gt_cap)
        F, A, K, dev = self.frames, self.max_agents, self.obj_cap, torch.device(device)
        self.boxes = torch.zeros((F, A, K, self.row_floats), dtype=torch.float32, device=dev)
        self.mask = torch.zeros((F, A, K), dtype=torch.uint8, device=dev)
        self.ids = torch.zeros((F, A, K), dtype=torch.int32, device=dev)
        self.transforms = torch.zeros((F, A, 4, 4), dtype=torch.float32, device=dev)
        self.agent_counts = torch.zeros((F,), dtype=torch.int32, device=dev)
        self.out = {"corners": torch.zeros((F, self.gt_cap, 8, 3), dtype=torch.float32, device=dev),
                    "labels": torch.zeros((F, self.gt_cap), dtype=torch.int32, device=dev) if multi else None,
                    "ids": torch.zeros((F, self.gt_cap), dtype=torch.int32, device=dev),
                    "counts": torch.zeros((F,), dtype=torch.int32, device=dev), "totals": torch.zeros((F,), dtype=torch.int32, device=dev)}

    def host_arrays(self, data_dicts):
        """the reference's per-frame ``data_dict``s (an ``OrderedDict`` of ``cav_content``) -> the five padded host arrays of the C entry.
        ``object_ids`` is a list aligned with the mask's set rows: it is scattered into their slots."""
        if len(data_dicts) > self.frames:
            raise ValueError(f"{len(data_dicts)} frames, the assembler holds {self.frames}")
        F, A, K = self.frames, self.max_agents, self.obj_cap
        boxes, mask = np.zeros((F, A, K, self.row_floats), np.float32), np.zeros((F, A, K), np.uint8)
        ids, tf, counts = np.zeros((F, A, K), np.int32), np.zeros((F, A, 4, 4), np.float32), np.zeros((F,), np.int32)
        host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)      # noqa: E731
        for f, data_dict in enumerate(data_dicts):
            if len(data_dict) > A:
                raise ValueError(f"frame {f}: {len(data_dict)} CAVs, max_agents is {A}")
            counts[f] = len(data_dict)
            for a, cav in enumerate(data_dict.values()):
                b, m = host(cav["object_bbx_center"]), host(cav["object_bbx_mask"]).reshape(-1) == 1
                if b.ndim != 2 or b.shape[1] != self.row_floats or b.shape[0] != m.shape[0]:
                    raise ValueError(f"frame {f}, CAV {a}: object_bbx_center {b.shape} with a mask of {m.shape[0]}: rows of {self.row_floats} floats expected")
                if m[K:].any():
                    raise ValueError(f"frame {f}, CAV {a}: a mask row set past obj_cap {K}")
                n = min(K, b.shape[0])
                boxes[f, a, :n], mask[f, a, :n] = b[:n], m[:n]
                if self.mode == 0:
                    oid = [int(v) for v in cav["object_ids"]]
                    if len(oid) != int(m.sum()):
                        raise ValueError(f"frame {f}, CAV {a}: {len(oid)} object_ids for {int(m.sum())} set mask rows")
                    if oid and not (-2 ** 31 <= min(oid) and max(oid) < 2 ** 31):
                        raise ValueError(f"frame {f}, CAV {a}: an object id outside int32")
                    ids[f, a, np.nonzero(m[:n])[0]] = oid
                tf[f, a] = host(cav[self.transform_key]).reshape(4, 4)
        return boxes, mask, ids, tf, counts

    def fill(self, data_dicts):
        """write the buffers in place (frames past ``len(data_dicts)`` become empty); -> self"""
        for dst, src in zip((self.boxes, self.mask, self.ids, self.transforms, self.agent_counts), self.host_arrays(data_dicts)):
            dst.copy_(torch.from_numpy(src))
        return self

    def __call__(self):
        """enqueue the kernel on the buffers as they are; nothing is read back -> the output dict (the same tensors every call)"""
        return gpu_gt_boxes_batch(self.boxes, self.mask, self.ids if self.mode == 0 else None, self.transforms, self.agent_counts,
                                  order=self.order, mode=self.mode, gt_range=self.gt_range, range_xy_only=self.range_xy_only,
                                  gt_cap=self.gt_cap, out=self.out)
