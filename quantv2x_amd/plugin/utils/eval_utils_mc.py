"""Per-class detection evaluation; mirror of ``opencood/utils/eval_utils_mc.py`` (``caluclate_tp_fp :41-93``, ``calculate_ap :95-133``,
``eval_final_results :136-159``).  The multi-class tools call ``caluclate_tp_fp`` once per class with that class's boxes and a
``result_stat`` of ``{threshold: {'tp': [], 'fp': [], 'gt': 0}}``: no range filter and no score list, and ``calculate_ap`` accumulates the
marks in the order they were appended (frame after frame, score order inside a frame) -- kept as it is.  The matching itself is
``eval_utils.caluclate_tp_fp``'s: CUDA tensors through ``qv2x_eval_tp_fp_f32``, CPU tensors / arrays through the numpy restatement."""
import os

from .eval_utils import _dump_yaml, ap_from_marks, caluclate_tp_fp as _tp_fp, voc_ap  # noqa: F401


def caluclate_tp_fp(det_boxes, det_score, gt_boxes, result_stat, iou_thresh):
    """Appends the frame's true / false positive marks (score order) and its GT count to ``result_stat[iou_thresh]``."""
    one = {iou_thresh: {'tp': [], 'fp': [], 'gt': 0, 'score': []}}
    _tp_fp(det_boxes, det_score, gt_boxes, one, iou_thresh)
    result_stat[iou_thresh]['fp'] += one[iou_thresh]['fp']
    result_stat[iou_thresh]['tp'] += one[iou_thresh]['tp']
    result_stat[iou_thresh]['gt'] += one[iou_thresh]['gt']


def calculate_ap(result_stat, iou):
    """AP, ``mrec``, ``mpre`` of ``result_stat[iou]`` in append order (eval_utils_mc.py:95-133).  As in the reference the ``tp`` / ``fp``
    lists of ``result_stat`` are left holding their cumulative sums.  Raises ZeroDivisionError without GT."""
    st = result_stat[iou]
    fp, tp = st['fp'], st['tp']
    assert len(fp) == len(tp)
    if st['gt'] == 0:
        raise ZeroDivisionError("calculate_ap: no ground truth")
    out = ap_from_marks(tp, fp, st['gt'])
    for marks in (fp, tp):
        run = 0
        for i, v in enumerate(marks):
            marks[i] += run
            run += v
    return out


def eval_final_results(result_stat, save_path):
    """``result_stat``: {class name: {threshold: {'tp', 'fp', 'gt'}}} -> {class name: {threshold: {'ap', 'mrec', 'mpre'}}}; prints the
    per-class AP and the mAP per threshold (eval_utils_mc.py:136-159, which returns nothing); ``save_path`` not None: writes ``eval.yaml``."""
    dump = {}
    for name, per_thr in result_stat.items():
        dump[name] = {}
        for thr in per_thr:
            ap, mrec, mpre = calculate_ap(per_thr, thr)
            dump[name][thr] = {"ap": ap, "mrec": mrec, "mpre": mpre}
            print(f'{name}: AP@{thr} is {ap:.4f}', end=' ')
        print("")
    names = list(result_stat)
    for thr in result_stat[names[0]]:
        print(f'mAP@{thr} is {sum(dump[n][thr]["ap"] for n in names) / len(names):.4f}', end=' ')
    if save_path is not None:
        flat = {f"{n}/{t}/{k}": v for n in dump for t in dump[n] for k, v in dump[n][t].items()}
        _dump_yaml(flat, os.path.join(save_path, 'eval.yaml'))
    return dump
