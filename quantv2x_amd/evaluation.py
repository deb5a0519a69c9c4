"""Detection evaluation on the device: ``qv2x_eval_tp_fp_f32`` behind a thin wrapper, and an evaluator that takes what ``PointsToBoxes``
returns and reports AP per (class, range, threshold) the way the reference's inference tools do (opencood/utils/eval_utils.py), without a
device-to-host copy per frame."""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import numpy as np
import torch

from .lib import EvalDesc, check, current_stream, load, ptr
from .plugin.utils.eval_utils import ap_from_marks

MAX_FRAMES, MAX_DET, MAX_GT = 64, 1024, 256
_workspaces = {}                                     # per descriptor and device: the call's workspace, kept between calls


def _desc(frames, det_cap, gt_cap, num_classes, ranges, thresholds) -> EvalDesc:
    if not 1 <= len(ranges) <= 4 or not 1 <= len(thresholds) <= 4:
        raise ValueError("1..4 ranges and 1..4 thresholds")
    d = EvalDesc()
    d.frames, d.det_cap, d.gt_cap, d.n_classes, d.n_ranges, d.n_thresholds = frames, det_cap, gt_cap, num_classes, len(ranges), len(thresholds)
    for i, (left, right) in enumerate(ranges):
        d.ranges[i][0], d.ranges[i][1] = float(left), float(right)
    for i, t in enumerate(thresholds):
        d.thresholds[i] = float(t)
    return d


def _dev_tensor(t, dtype, dev, shape, name):
    if t is None:
        return None
    t = torch.as_tensor(t)
    if t.device != dev or t.dtype != dtype or not t.is_contiguous():
        t = t.to(device=dev, dtype=dtype, non_blocking=True).contiguous()
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} {tuple(t.shape)}: {shape} expected")
    return t


def gpu_tp_fp_batch(det_corners, det_scores, det_labels, det_counts, gt_corners, gt_labels, gt_counts, *, thresholds: Sequence[float],
                    ranges: Sequence[Sequence[float]], num_classes: int = 0):
    """One ``qv2x_eval_tp_fp_f32`` call (include/qv2x.h has the conventions).  ``det_corners`` f32 [frames, det_cap, 8, 3], ``det_scores``
    f32 [frames, det_cap], ``det_labels`` i32 [frames, det_cap], ``det_counts`` i32 [frames]; ``gt_corners`` f32 [frames, gt_cap, 8, 3],
    ``gt_labels`` i32 [frames, gt_cap], ``gt_counts`` i32 [frames], all on one GPU (labels may be None with ``num_classes`` 0).  Range bounds
    and thresholds are rounded to float32.  Nothing is read back and nothing waits: -> (order i32 [frames, det_cap], scores f32
    [frames, det_cap], flags u8 [frames, P, det_cap], match i32 [frames, P, det_cap], gt i32 [frames, P]) on the GPU, P = max(1,
    num_classes) * len(ranges) * len(thresholds) with the threshold fastest."""
    lib = load()
    dev = det_corners.device
    if dev.type != "cuda":
        raise ValueError("gpu_tp_fp_batch: tensors on the GPU expected (the CPU path is plugin.utils.eval_utils.tp_fp_frame)")
    frames, det_cap, gt_cap = int(det_corners.shape[0]), int(det_corners.shape[1]), int(gt_corners.shape[1])
    d = _desc(frames, det_cap, gt_cap, int(num_classes), ranges, thresholds)
    det_corners = _dev_tensor(det_corners, torch.float32, dev, (frames, det_cap, 8, 3), "det_corners")
    det_scores = _dev_tensor(det_scores, torch.float32, dev, (frames, det_cap), "det_scores")
    det_counts = _dev_tensor(det_counts, torch.int32, dev, (frames,), "det_counts")
    gt_corners = _dev_tensor(gt_corners, torch.float32, dev, (frames, gt_cap, 8, 3), "gt_corners")
    gt_counts = _dev_tensor(gt_counts, torch.int32, dev, (frames,), "gt_counts")
    if num_classes > 0:
        det_labels = _dev_tensor(det_labels, torch.int32, dev, (frames, det_cap), "det_labels")
        gt_labels = _dev_tensor(gt_labels, torch.int32, dev, (frames, gt_cap), "gt_labels")
    else:
        det_labels = gt_labels = None
    need = lib.qv2x_eval_workspace_bytes(C.byref(d))
    if need < 0:
        check(-1, "qv2x_eval_workspace_bytes")
    key = (dev, bytes(d))
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    P = max(1, int(num_classes)) * len(ranges) * len(thresholds)
    order = torch.empty((frames, det_cap), dtype=torch.int32, device=dev)
    scores = torch.empty((frames, det_cap), dtype=torch.float32, device=dev)
    flags = torch.empty((frames, P, det_cap), dtype=torch.uint8, device=dev)
    match = torch.empty((frames, P, det_cap), dtype=torch.int32, device=dev)
    gt = torch.empty((frames, P), dtype=torch.int32, device=dev)
    check(lib.qv2x_eval_tp_fp_f32(C.byref(d), ptr(det_corners), ptr(det_scores), ptr(det_labels), ptr(det_counts), ptr(gt_corners),
                                  ptr(gt_labels), ptr(gt_counts), ptr(ws), need, ptr(order), ptr(scores), ptr(flags), ptr(match), ptr(gt),
                                  current_stream()), "qv2x_eval_tp_fp_f32")
    return order, scores, flags, match, gt


class DetectionEvaluator:
    """AP over a run of frames.  ``update`` enqueues the kernels of one batch and keeps their outputs on the device -- no read-back, no
    synchronisation; ``result`` reads everything back once and does the reference's ``calculate_ap`` / ``voc_ap`` arithmetic
    (eval_utils.py:124-166: marks of all frames ordered by descending score, a stable sort here; cumulative sums; float64).  Each mark
    is paired with its own detection's score (the reference pairs them only when the detections arrive sorted, which they do)."""

    def __init__(self, thresholds=(0.3, 0.5, 0.7), ranges=((-math.inf, math.inf), (0, 30), (30, 50), (50, 100)), num_classes=0, max_gt=256):
        if not 1 <= max_gt <= MAX_GT:
            raise ValueError(f"max_gt in 1..{MAX_GT}")
        self.thresholds, self.ranges = tuple(float(t) for t in thresholds), tuple((float(a), float(b)) for a, b in ranges)
        self.num_classes, self.max_gt = int(num_classes), int(max_gt)
        _desc(1, 1, 1, self.num_classes, self.ranges, self.thresholds)
        self.reset()

    def reset(self):
        self._parts = []                                 # per update: (scores [F, cap], flags [F, P, cap], gt [F, P]) on the device

    def update(self, out: dict, gt_corners, gt_labels, gt_counts):
        """``out``: what ``PointsToBoxes.__call__`` returns (``corners`` / ``scores`` / ``labels`` / ``counts`` on the device);
        ``gt_corners`` f32 [frames, G, 8, 3] with G <= ``max_gt``, ``gt_labels`` i32 [frames, G] (None with ``num_classes`` 0), ``gt_counts`` i32
        [frames], on the same device.  More than 64 frames go in calls of 64."""
        frames = int(out["corners"].shape[0])
        if int(gt_corners.shape[1]) > self.max_gt:
            raise ValueError(f"{int(gt_corners.shape[1])} GT rows per frame, max_gt is {self.max_gt}")
        for f0 in range(0, frames, MAX_FRAMES):
            s = slice(f0, min(frames, f0 + MAX_FRAMES))
            _, scores, flags, _, gt = gpu_tp_fp_batch(
                out["corners"][s], out["scores"][s], out["labels"][s] if self.num_classes > 0 else None, out["counts"][s], gt_corners[s],
                gt_labels[s] if self.num_classes > 0 else None, gt_counts[s], thresholds=self.thresholds, ranges=self.ranges,
                num_classes=self.num_classes)
            self._parts.append((scores, flags, gt))

    def update_from(self, out: dict, gt: dict):
        """``update`` on what ``ground_truth.gpu_gt_boxes_batch`` / ``GroundTruthAssembler`` return (``corners`` / ``labels`` / ``counts`` on the
        device): nothing is read back in between.  A frame whose ``totals`` exceed its ``counts`` is evaluated on the rows that were written."""
        if self.num_classes > 0 and gt.get("labels") is None:
            raise ValueError("num_classes > 0 needs ground-truth labels (8-float object rows)")
        self.update(out, gt["corners"], gt.get("labels"), gt["counts"])

    def result(self) -> dict:
        """-> ``ap`` f64, ``tp`` / ``fp`` / ``gt`` i64 arrays [classes, ranges, thresholds] (classes = max(1, num_classes)) and ``mrec`` /
        ``mpre``: nested lists of the same shape holding the curves.  A problem without GT reports ``ap`` nan and empty curves (the
        reference divides by zero there)."""
        C_, R, T = max(1, self.num_classes), len(self.ranges), len(self.thresholds)
        P = C_ * R * T
        score_l, flag_l, gt_total = [], [], np.zeros((P,), np.int64)
        if self._parts:
            # one device buffer, one copy
            sizes = [(s.shape, f.shape, g.shape) for s, f, g in self._parts]
            blob = torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for part in self._parts for t in part]).cpu().numpy()
            at = 0
            for ss, fs, gs in sizes:
                n = int(np.prod(ss)) * 4
                score_l.append(np.frombuffer(blob[at:at + n].tobytes(), np.float32).reshape(ss)); at += n
                n = int(np.prod(fs))
                flag_l.append(blob[at:at + n].reshape(fs)); at += n
                n = int(np.prod(gs)) * 4
                gt_total += np.frombuffer(blob[at:at + n].tobytes(), np.int32).reshape(gs).sum(0); at += n
        ap = np.full((P,), np.nan)
        tp_n, fp_n = np.zeros((P,), np.int64), np.zeros((P,), np.int64)
        mrec, mpre = [[] for _ in range(P)], [[] for _ in range(P)]
        for p in range(P):
            sc, fl = [], []
            for scores, flags in zip(score_l, flag_l):               # frame after frame, rank order inside a frame
                m = flags[:, p, :] != 0
                sc.append(scores[m]); fl.append(flags[:, p, :][m])
            sc = np.concatenate(sc) if sc else np.zeros((0,), np.float32)
            fl = np.concatenate(fl) if fl else np.zeros((0,), np.uint8)
            tp_n[p], fp_n[p] = int((fl == 2).sum()), int((fl == 1).sum())
            if gt_total[p] > 0:
                idx = np.argsort(-sc, kind="stable")
                ap[p], mrec[p], mpre[p] = ap_from_marks((fl[idx] == 2), (fl[idx] == 1), int(gt_total[p]))
        nest = lambda v: [[[v[(c * R + r) * T + t] for t in range(T)] for r in range(R)] for c in range(C_)]   # noqa: E731
        return {"ap": ap.reshape(C_, R, T), "tp": tp_n.reshape(C_, R, T), "fp": fp_n.reshape(C_, R, T), "gt": gt_total.reshape(C_, R, T),
                "mrec": nest(mrec), "mpre": nest(mpre)}
