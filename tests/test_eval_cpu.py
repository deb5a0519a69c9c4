"""The detection evaluator without a GPU: the plugin's CPU path (``quantv2x_amd/plugin/utils/eval_utils.py`` / ``eval_utils_mc.py``)
reproduces what the reference's own evaluator gave on tests/golden/eval.npz (tests/golden/make_golden_eval.py: control flow pinned,
polygon areas unpinned), the new C entries reject bad arguments on the host, and the corner cases of the Python surface."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from quantv2x_amd.plugin.utils import eval_utils, eval_utils_mc


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden["eval"]


def _frames(fx):
    for f in range(fx["det_corners"].shape[0]):
        n, g = int(fx["det_counts"][f]), int(fx["gt_counts"][f])
        yield (fx["det_corners"][f, :n], fx["det_scores"][f, :n], fx["det_labels"][f, :n], fx["gt_corners"][f, :g], fx["gt_labels"][f, :g])


def test_cpu_path_reproduces_the_reference_per_range(fx):
    thresholds, ranges = [float(t) for t in fx["thresholds"]], [tuple(float(v) for v in r) for r in fx["ranges"]]
    for ri, (left, right) in enumerate(ranges):
        stat = {t: {"tp": [], "fp": [], "gt": 0, "score": []} for t in thresholds}
        for k, (det, sc, _, gt, _) in enumerate(_frames(fx)):
            for t in thresholds:
                if k % 2:                                             # tensors and arrays both
                    eval_utils.caluclate_tp_fp(torch.from_numpy(det), torch.from_numpy(sc), torch.from_numpy(gt), stat, t, left, right)
                else:
                    eval_utils.caluclate_tp_fp(det, sc, gt, stat, t, left_range=left, right_range=right)
        for ti, t in enumerate(thresholds):
            k = f"r{ri}_t{ti}"
            assert stat[t]["tp"] == fx["tp_" + k].tolist() and stat[t]["fp"] == fx["fp_" + k].tolist(), k
            assert stat[t]["gt"] == int(fx["gt_" + k]), k
            np.testing.assert_array_equal(np.array(stat[t]["score"], np.float32), fx["score_" + k])
            ap, mrec, mpre = eval_utils.calculate_ap(stat, t)
            assert abs(ap - float(fx["ap_" + k])) <= 1e-12, k
            np.testing.assert_allclose(mrec, fx["mrec_" + k], rtol=0, atol=1e-12)
            np.testing.assert_allclose(mpre, fx["mpre_" + k], rtol=0, atol=1e-12)
    # the full range is what eval_final_results reports
    stat = {t: {"tp": [], "fp": [], "gt": 0, "score": []} for t in (0.3, 0.5, 0.7)}
    for det, sc, _, gt, _ in _frames(fx):
        for t in stat:
            eval_utils.caluclate_tp_fp(det, sc, gt, stat, t)
    got = eval_utils.eval_final_results(stat, None)
    assert np.abs(np.array(got) - np.array([float(fx[f"ap_r0_t{ti}"]) for ti in range(3)])).max() <= 1e-12


def test_cpu_path_reproduces_the_reference_per_class(fx):
    thresholds = [float(t) for t in fx["thresholds"]]
    for c in (1, 2, 3):
        stat = {t: {"tp": [], "fp": [], "gt": 0} for t in thresholds}
        for det, sc, dl, gt, gl in _frames(fx):
            dm, gm = dl == c, gl == c
            for t in thresholds:
                eval_utils_mc.caluclate_tp_fp(det[dm] if dm.any() else None, sc[dm], gt[gm], stat, t)
        for ti, t in enumerate(thresholds):
            k = f"c{c}_t{ti}"
            assert stat[t]["tp"] == fx["mc_tp_" + k].tolist() and stat[t]["fp"] == fx["mc_fp_" + k].tolist(), k
            assert stat[t]["gt"] == int(fx["mc_gt_" + k]), k
            ap, mrec, mpre = eval_utils_mc.calculate_ap(stat, t)
            assert abs(ap - float(fx["mc_ap_" + k])) <= 1e-12, k
            np.testing.assert_allclose(mrec, fx["mc_mrec_" + k], rtol=0, atol=1e-12)
            np.testing.assert_allclose(mpre, fx["mc_mpre_" + k], rtol=0, atol=1e-12)


def test_all_problems_at_once_equal_the_single_problem_calls(fx):
    """``tp_fp_frame`` (every class, range and threshold of a frame: the layout of qv2x_eval_tp_fp_f32) against the golden per-range lists"""
    thresholds, ranges = [float(t) for t in fx["thresholds"]], [tuple(float(v) for v in r) for r in fx["ranges"]]
    tp = {(ri, ti): [] for ri in range(4) for ti in range(3)}
    gt_n = {k: 0 for k in tp}
    for det, sc, _, gt, _ in _frames(fx):
        one = eval_utils.tp_fp_frame(det, sc, gt, thresholds, ranges)
        assert one["flags"].shape == (12, len(sc)) and one["order"].tolist() == list(range(len(sc)))      # stored in score order
        for (ri, ti) in tp:
            fl = one["flags"][ri * 3 + ti]
            tp[ri, ti] += (fl[fl != 0] == 2).astype(int).tolist()
            gt_n[ri, ti] += int(one["gt"][ri * 3 + ti])
            m = one["match"][ri * 3 + ti]
            assert ((m >= 0) == (fl == 2)).all() and len(set(m[m >= 0].tolist())) == int((m >= 0).sum())   # a GT is matched once
    for (ri, ti) in tp:
        assert tp[ri, ti] == fx[f"tp_r{ri}_t{ti}"].tolist() and gt_n[ri, ti] == int(fx[f"gt_r{ri}_t{ti}"])


def test_no_detections_and_no_gt():
    box = np.zeros((1, 8, 3), np.float32)
    box[0, :4, :2] = [[1, -1], [1, 1], [-1, 1], [-1, -1]]
    box[0, :, 0] += 10.0
    stat = {0.5: {"tp": [], "fp": [], "gt": 0, "score": []}}
    eval_utils.caluclate_tp_fp(None, None, torch.from_numpy(np.repeat(box, 3, 0)), stat, 0.5)     # det_boxes None: every GT counts, range or not
    assert stat[0.5] == {"tp": [], "fp": [], "gt": 3, "score": []}
    eval_utils.caluclate_tp_fp(box, np.array([0.9], np.float32), np.zeros((0, 8, 3), np.float32), stat, 0.5)   # a frame without GT
    assert stat[0.5]["tp"] == [0] and stat[0.5]["fp"] == [1] and stat[0.5]["gt"] == 3 and stat[0.5]["score"] == [np.float32(0.9)]
    eval_utils.caluclate_tp_fp(box, np.array([0.8], np.float32), box, stat, 0.5, 20.0, 30.0)    # out of range on both sides
    assert stat[0.5]["tp"] == [0] and stat[0.5]["gt"] == 3
    eval_utils.caluclate_tp_fp(box[:, :4, :2], np.array([0.7], np.float32), box[:, :4, :2], stat, 0.5, 0.0, 30.0)   # (N, 4, 2) boxes
    assert stat[0.5]["tp"] == [0, 1] and stat[0.5]["fp"] == [1, 0] and stat[0.5]["gt"] == 4
    ap, mrec, mpre = eval_utils.calculate_ap(stat, 0.5)
    assert ap == 0.25 * 0.5 and mrec == [0.0, 0.0, 0.25, 1.0] and mpre == [0.5, 0.5, 0.5, 0.0]
    with pytest.raises(ZeroDivisionError):
        eval_utils.calculate_ap({0.5: {"tp": [], "fp": [], "gt": 0, "score": []}}, 0.5)


def test_evaluator_without_gt_reports_nan():
    from quantv2x_amd.evaluation import DetectionEvaluator
    ev = DetectionEvaluator(num_classes=3)
    r = ev.result()
    assert r["ap"].shape == (3, 4, 3) and np.isnan(r["ap"]).all() and (r["gt"] == 0).all() and (r["tp"] == 0).all()
    assert r["mrec"][2][3][2] == [] and r["mpre"][0][0][0] == []
    ev.reset()
    assert np.isnan(DetectionEvaluator(thresholds=(0.5,), ranges=((-math.inf, math.inf),)).result()["ap"]).all()
    with pytest.raises(ValueError):
        DetectionEvaluator(max_gt=257)
    with pytest.raises(ValueError):
        DetectionEvaluator(thresholds=(0.1, 0.2, 0.3, 0.4, 0.5))


def test_eval_final_results_writes_only_when_given_a_path(fx, tmp_path):
    stat = {t: {"tp": [1, 0], "fp": [0, 1], "gt": 2, "score": [0.9, 0.8]} for t in (0.3, 0.5, 0.7)}
    assert eval_utils.eval_final_results(stat, None) == (0.5, 0.5, 0.5)
    assert eval_utils.eval_final_results(stat, str(tmp_path), infer_info="x") == (0.5, 0.5, 0.5)
    text = (tmp_path / "eval_x.yaml").read_text()
    assert "ap_50: 0.5" in text and "mrec_70:" in text
    mc = {"car": {0.5: {"tp": [1, 0], "fp": [0, 1], "gt": 2}}, "truck": {0.5: {"tp": [], "fp": [], "gt": 1}}}
    out = eval_utils_mc.eval_final_results(mc, str(tmp_path))
    assert out["car"][0.5]["ap"] == 0.5 and out["truck"][0.5]["ap"] == 0.0 and (tmp_path / "eval.yaml").exists()


def test_argument_errors_of_the_eval_entries_without_gpu():
    from quantv2x_amd import build, lib
    build.build()
    l = lib.load()
    assert C.sizeof(lib.EvalDesc) == 6 * 4 + 8 * 4 + 4 * 4

    def desc(**kw):
        d = lib.EvalDesc()
        d.frames, d.det_cap, d.gt_cap, d.n_classes, d.n_ranges, d.n_thresholds = 2, 100, 40, 0, 1, 1
        d.ranges[0][0], d.ranges[0][1], d.thresholds[0] = -math.inf, math.inf, 0.5
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    need = l.qv2x_eval_workspace_bytes(C.byref(desc()))
    assert need >= 2 * 100 * 40 * 4 + 2 * 100 * 4 + 2 * 40 * 4 and need % 256 == 0
    assert l.qv2x_eval_workspace_bytes(None) == -1
    for bad in (dict(frames=0), dict(frames=65), dict(det_cap=0), dict(det_cap=1025), dict(gt_cap=0), dict(gt_cap=257), dict(n_classes=-1),
                dict(n_classes=5), dict(n_ranges=0), dict(n_ranges=5), dict(n_thresholds=0), dict(n_thresholds=5)):
        assert l.qv2x_eval_workspace_bytes(C.byref(desc(**bad))) == -1, bad
        assert next(iter(bad)).split("_")[-1].rstrip("s") in l.qv2x_last_error().decode(), (bad, l.qv2x_last_error())
    buf = np.zeros(need + 512, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 256
    p, ws = C.c_void_p(base), C.c_void_p(base)

    def call(d, args=None, ws=ws, ws_bytes=need):
        a = [p] * 7 if args is None else args
        return l.qv2x_eval_tp_fp_f32(C.byref(d), *a, ws, ws_bytes, p, p, p, p, p, None)
    for thr in (0.0, -0.1, 1.0000001, math.nan):
        d = desc()
        d.thresholds[0] = thr
        assert call(d) == -1 and b"threshold" in l.qv2x_last_error()
    d = desc()
    d.ranges[0][0] = math.nan
    assert call(d) == -1 and b"range" in l.qv2x_last_error()
    for i in (0, 1, 3, 4, 6):                                         # corners, scores, counts: never optional
        a = [p] * 7
        a[i] = None
        assert call(desc(), a) == -1 and b"null" in l.qv2x_last_error()
    for i in (2, 5):                                                  # labels: optional only when class-agnostic
        a = [p] * 7
        a[i] = None
        assert call(desc(n_classes=3), a) == -1 and b"labels" in l.qv2x_last_error()
    assert l.qv2x_eval_tp_fp_f32(C.byref(desc()), *([p] * 7), ws, need, p, p, None, p, p, None) == -1      # an output
    assert call(desc(), ws=None) == -1
    assert call(desc(), ws_bytes=need - 1) == -1 and b"workspace" in l.qv2x_last_error()
    assert call(desc(), ws=C.c_void_p(base + 64)) == -2 and b"aligned" in l.qv2x_last_error()


def test_eval_utils_resolve_through_the_shim():
    """``opencood.utils.eval_utils`` / ``eval_utils_mc`` with ``integration/`` on the path and no reference tree: the mirror's objects"""
    script = ("import sys\nassert not any('reference' in p for p in sys.path), sys.path\n"
              "from opencood.utils.eval_utils import voc_ap, caluclate_tp_fp, calculate_ap, eval_final_results\n"
              "from opencood.utils import eval_utils_mc\n"
              "import quantv2x_amd.plugin.utils.eval_utils as m, quantv2x_amd.plugin.utils.eval_utils_mc as mc\n"
              "assert caluclate_tp_fp is m.caluclate_tp_fp and voc_ap is m.voc_ap and eval_final_results is m.eval_final_results\n"
              "assert eval_utils_mc.caluclate_tp_fp is mc.caluclate_tp_fp and eval_utils_mc.calculate_ap is mc.calculate_ap\n"
              "print('shim ok')\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "integration"), ROOT])
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "shim ok" in r.stdout, r.stderr[-2000:]
