"""Detection evaluation; mirror of ``opencood/utils/eval_utils.py`` (``voc_ap :14-37``, ``caluclate_tp_fp :40-120``, ``calculate_ap
:124-166``, ``eval_final_results :169-194``) with the reference's names, spelling and signatures.

``caluclate_tp_fp`` sends CUDA tensors through ``quantv2x_amd.evaluation.gpu_tp_fp_batch`` (``qv2x_eval_tp_fp_f32``, one frame, one
problem) and CPU tensors / arrays through ``tp_fp_frame`` below, a numpy restatement of the same conventions (include/qv2x.h):

* order: stable descending score, equal scores keep the lower row first (the reference's ``np.argsort(-score)`` is unstable);
* centre: the four bottom-face corners summed in index order times 0.25, float64; membership ``left < distance < right``;
* IoU: ``float32(inter / union)`` in float64, convex clipping of the two quadrilaterals (the reference takes both areas from shapely,
  which is not vendored: the areas are unpinned, as for the NMS), 0 for disjoint bounding boxes or an empty union;
* matching: greedy in rank order, largest IoU among the GT not yet matched, ties to the lowest GT row, ``iou < float32(threshold)`` is a
  false positive.

The reference quirk is kept: ``result_stat[...]['score']`` receives the frame's in-range scores in INPUT order while ``tp`` / ``fp`` are in
score order; the two agree when the detections arrive sorted, which is how every post-processor delivers them."""
import os

import numpy as np


def voc_ap(rec, prec):
    """VOC 2010 average precision of a recall / precision curve (lists; both are extended in place, as in the reference)."""
    rec.insert(0, 0.0)
    rec.append(1.0)
    prec.insert(0, 0.0)
    prec.append(0.0)
    mrec, mpre = rec[:], prec[:]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap, mrec, mpre


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------------
def _signed_area2(poly):
    s = 0.0
    n = len(poly)
    for i in range(n):
        x0, y0 = poly[i]
        x1, y1 = poly[(i + 1) % n]
        s += x0 * y1 - x1 * y0
    return s


def quad_inter_area(p, q):
    """area of the intersection of two convex quadrilaterals (float64, any orientation): Sutherland-Hodgman, the operations of
    csrc/quad_iou.h in the same order"""
    clip = [(float(v[0]), float(v[1])) for v in q]
    qa = _signed_area2(clip)
    if qa == 0.0:                                                  # a clip polygon without area (a point: four zero-length edges clip nothing)
        return 0.0
    if qa < 0.0:
        clip = clip[::-1]
    out = [(float(v[0]), float(v[1])) for v in p]
    for i in range(4):
        if not out:
            break
        ax, ay = clip[i]
        bx, by = clip[(i + 1) % 4]
        inp, out = out, []
        for j in range(len(inp)):
            cx, cy = inp[j]
            dx, dy = inp[(j + 1) % len(inp)]
            sc = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            sd = (bx - ax) * (dy - ay) - (by - ay) * (dx - ax)
            if sc >= 0.0:
                out.append((cx, cy))
            if (sc >= 0.0) != (sd >= 0.0):
                t = sc / (sc - sd)
                out.append((cx + t * (dx - cx), cy + t * (dy - cy)))
    return abs(0.5 * _signed_area2(out)) if len(out) >= 3 else 0.0


def quad_area(p):
    return abs(0.5 * _signed_area2([(float(v[0]), float(v[1])) for v in p]))


def _quads(boxes):
    """(N, 8, 3) or (N, 4, 2) boxes -> float64 [N, 4, 2]: x, y of the bottom face"""
    b = np.asarray(boxes)
    if b.ndim != 3 or b.shape[1] < 4 or b.shape[2] < 2:
        raise ValueError(f"boxes {b.shape}: (N, 8, 3) or (N, 4, 2) expected")
    return b[:, :4, :2].astype(np.float64)


def centre_distance(quads):
    """float64 [N]: distance of the bottom face's centre from the origin"""
    cx = (quads[:, 0, 0] + quads[:, 1, 0] + quads[:, 2, 0] + quads[:, 3, 0]) * 0.25
    cy = (quads[:, 0, 1] + quads[:, 1, 1] + quads[:, 2, 1] + quads[:, 3, 1]) * 0.25
    return np.sqrt(cx * cx + cy * cy)


def iou_matrix(det_quads, gt_quads):
    """float32 [N, G].  The bounding-box test is vectorized; only the pairs it lets through are clipped."""
    n, g = det_quads.shape[0], gt_quads.shape[0]
    out = np.zeros((n, g), np.float32)
    if n == 0 or g == 0:
        return out
    dlo, dhi, glo, ghi = det_quads.min(1), det_quads.max(1), gt_quads.min(1), gt_quads.max(1)
    apart = ((dhi[:, None, 0] < glo[None, :, 0]) | (ghi[None, :, 0] < dlo[:, None, 0]) |
             (dhi[:, None, 1] < glo[None, :, 1]) | (ghi[None, :, 1] < dlo[:, None, 1]))
    da = [quad_area(q) for q in det_quads]
    ga = [quad_area(q) for q in gt_quads]
    for i, j in zip(*np.nonzero(~apart)):
        inter = quad_inter_area(det_quads[i], gt_quads[j])
        union = da[i] + ga[j] - inter
        out[i, j] = np.float32(inter / union) if union > 0.0 else np.float32(0.0)
    return out


def tp_fp_frame(det_boxes, det_score, gt_boxes, thresholds, ranges, det_labels=None, gt_labels=None, num_classes=0):
    """One frame, every (class, range, threshold) problem: what ``qv2x_eval_tp_fp_f32`` writes for it, as numpy arrays.
    -> dict: ``order`` i32 [N] (row at rank r), ``scores`` f32 [N], ``iou`` f32 [N, G] by rank, ``flags`` u8 [P, N] (0 not in the problem,
    1 false positive, 2 true positive), ``match`` i32 [P, N] (GT row or -1), ``gt`` i32 [P]; P = max(1, num_classes) * len(ranges) *
    len(thresholds), threshold fastest."""
    dq, gq = _quads(det_boxes), _quads(gt_boxes)
    score = np.asarray(det_score, dtype=np.float32).reshape(-1)
    n, g = dq.shape[0], gq.shape[0]
    order = np.argsort(-score, kind="stable").astype(np.int32)
    dq = dq[order]
    iou = iou_matrix(dq, gq)
    dd, gd = centre_distance(dq), centre_distance(gq)
    if num_classes > 0:
        dl, gl = np.asarray(det_labels).reshape(-1)[order], np.asarray(gt_labels).reshape(-1)
    n_sets = max(1, num_classes) * len(ranges)
    P = n_sets * len(thresholds)
    flags, match, gt_n = np.zeros((P, n), np.uint8), np.full((P, n), -1, np.int32), np.zeros((P,), np.int32)
    for c in range(max(1, num_classes)):
        for ri, (left, right) in enumerate(ranges):
            din, gin = (left < dd) & (dd < right), (left < gd) & (gd < right)
            if num_classes > 0:
                din, gin = din & (dl == c + 1), gin & (gl == c + 1)
            for ti, thr in enumerate(thresholds):
                p = (c * len(ranges) + ri) * len(thresholds) + ti
                gt_n[p] = int(gin.sum())
                alive = np.nonzero(gin)[0]                            # ascending rows: the first maximum is the lowest row
                thr32 = np.float32(thr)
                for r in np.nonzero(din)[0]:
                    k = int(np.argmax(iou[r, alive])) if alive.size else -1
                    if k < 0 or iou[r, alive[k]] < thr32:
                        flags[p, r] = 1
                    else:
                        flags[p, r], match[p, r] = 2, alive[k]
                        alive = np.delete(alive, k)
    return {"order": order, "scores": score[order], "iou": iou, "flags": flags, "match": match, "gt": gt_n}


def _to_numpy(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _is_cuda(t):
    return bool(getattr(t, "is_cuda", False))


def _gpu_one_problem(det_boxes, det_score, gt_boxes, iou_thresh, left_range, right_range):
    """one frame, one problem through ``gpu_tp_fp_batch`` -> (flags u8 [N] by rank, order [N], gt count)"""
    import torch
    from quantv2x_amd.evaluation import gpu_tp_fp_batch
    dev = det_boxes.device
    n, g = int(det_boxes.shape[0]), int(gt_boxes.shape[0])

    def frame(boxes, rows):
        c = torch.zeros((1, max(rows, 1), 8, 3), dtype=torch.float32, device=dev)
        if rows:
            c[0, :, :4, :2] = boxes[:, :4, :2].to(device=dev, dtype=torch.float32)
        return c
    scores = torch.zeros((1, max(n, 1)), dtype=torch.float32, device=dev)
    if n:
        scores[0] = det_score.reshape(-1).to(device=dev, dtype=torch.float32)
    out = gpu_tp_fp_batch(frame(det_boxes, n), scores, None, torch.full((1,), n, dtype=torch.int32, device=dev),
                          frame(gt_boxes, g), None, torch.full((1,), g, dtype=torch.int32, device=dev),
                          thresholds=(iou_thresh,), ranges=((left_range, right_range),), num_classes=0)
    order, _, flags, _, gt_n = out
    return flags[0, 0, :n].cpu().numpy(), order[0, :n].cpu().numpy(), int(gt_n[0, 0])


def caluclate_tp_fp(det_boxes, det_score, gt_boxes, result_stat, iou_thresh, left_range=-float('inf'), right_range=float('inf')):
    """Appends the frame's true / false positive marks (score order), its in-range scores and its GT count to
    ``result_stat[iou_thresh]`` (eval_utils.py:40-120).  ``det_boxes`` / ``gt_boxes``: (N, 8, 3) or (N, 4, 2) tensors or arrays;
    ``det_boxes`` None: a frame without detections, every GT counts."""
    fp, tp = [], []
    gt = int(gt_boxes.shape[0])
    if det_boxes is not None:
        if _is_cuda(det_boxes):
            flags, order, gt = _gpu_one_problem(det_boxes, det_score, gt_boxes, iou_thresh, left_range, right_range)
            score = _to_numpy(det_score).reshape(-1)
        else:
            score = _to_numpy(det_score).reshape(-1)
            one = tp_fp_frame(_to_numpy(det_boxes), score, _to_numpy(gt_boxes), (iou_thresh,), ((left_range, right_range),))
            flags, order, gt = one["flags"][0], one["order"], int(one["gt"][0])
        member = flags != 0
        tp = [int(v == 2) for v in flags[member]]
        fp = [int(v == 1) for v in flags[member]]
        result_stat[iou_thresh]['score'] += np.asarray(score)[np.sort(order[member])].tolist()
    result_stat[iou_thresh]['fp'] += fp
    result_stat[iou_thresh]['tp'] += tp
    result_stat[iou_thresh]['gt'] += gt


def ap_from_marks(tp, fp, gt_total):
    """cumulative sums, recall = tp / gt, precision = tp / (tp + fp), then ``voc_ap`` -- float64, the reference's operations in its order
    (eval_utils.py:146-164); ``tp`` / ``fp``: 0 / 1 marks in evaluation order"""
    tp, fp = np.cumsum(np.asarray(tp, np.int64)), np.cumsum(np.asarray(fp, np.int64))
    rec = (tp.astype(np.float64) / gt_total).tolist()
    prec = (tp.astype(np.float64) / (fp + tp)).tolist()
    return voc_ap(rec, prec)


def calculate_ap(result_stat, iou):
    """AP, ``mrec``, ``mpre`` of ``result_stat[iou]`` (eval_utils.py:124-166): marks ordered by descending score over all frames (a stable
    sort here), then ``ap_from_marks``.  Raises ZeroDivisionError without GT, as the reference."""
    st = result_stat[iou]
    fp, tp, score = np.array(st['fp']), np.array(st['tp']), np.array(st['score'])
    assert len(fp) == len(tp) and len(tp) == len(score)
    if st['gt'] == 0:
        raise ZeroDivisionError("calculate_ap: no ground truth")
    idx = np.argsort(-score, kind="stable")
    return ap_from_marks(tp[idx], fp[idx], st['gt'])


def _dump_yaml(d, path):
    """flat ``key: scalar`` / ``key: [list]`` file (what the reference's yaml dump of this dict holds), no yaml package needed"""
    with open(path, "w") as fh:
        for k, v in d.items():
            if isinstance(v, (list, tuple)):
                fh.write(f"{k}:\n" + "".join(f"- {float(e)!r}\n" for e in v))
            else:
                fh.write(f"{k}: {float(v)!r}\n")


def eval_final_results(result_stat, save_path, infer_info=None):
    """AP at IoU 0.3 / 0.5 / 0.7 of ``result_stat`` (eval_utils.py:169-194): prints and returns them; ``save_path`` not None: also writes
    ``eval.yaml`` / ``eval_<infer_info>.yaml`` there."""
    ap_30, _, _ = calculate_ap(result_stat, 0.30)
    ap_50, mrec_50, mpre_50 = calculate_ap(result_stat, 0.50)
    ap_70, mrec_70, mpre_70 = calculate_ap(result_stat, 0.70)
    if save_path is not None:
        dump = {'ap30': ap_30, 'ap_50': ap_50, 'ap_70': ap_70, 'mpre_50': mpre_50, 'mrec_50': mrec_50, 'mpre_70': mpre_70, 'mrec_70': mrec_70}
        _dump_yaml(dump, os.path.join(save_path, 'eval.yaml' if infer_info is None else f'eval_{infer_info}.yaml'))
    print(infer_info, 'The Average Precision at IOU 0.3 is %.4f, The Average Precision at IOU 0.5 is %.4f, '
          'The Average Precision at IOU 0.7 is %.4f' % (ap_30, ap_50, ap_70))
    return ap_30, ap_50, ap_70
