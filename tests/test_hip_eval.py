"""``qv2x_eval_tp_fp_f32`` on the GPU against the plugin's CPU path (``plugin/utils/eval_utils.py:tp_fp_frame``, itself pinned against the
reference's evaluator by tests/test_eval_cpu.py): order, flags, matches and GT counts of every problem identical, at the smallest shapes
where the kernels take another path -- a wave's 64 lanes and its four GT slots per lane (GT counts 63 / 64 / 65 / 256), the 64-rank
chunks of the walk and the 256-row blocks of the rank pass (130 and 1000 detections), empty and full frames.  Random inputs keep the
fixture's margins (asserted, reseeded until they hold): no IoU within 1e-4 of a threshold, no centre within 1e-3 m of a range bound, and
distinct scores except where a tie is the point."""
import functools
import math

import numpy as np
import pytest
import torch

from quantv2x_amd.plugin.utils import eval_utils

pytestmark = pytest.mark.gpu

INF = math.inf
THRESHOLDS = (0.3, 0.5, 0.7)
RANGES = ((-INF, INF), (0.0, 30.0), (30.0, 50.0), (50.0, 100.0))
SIZES = ((4.2, 1.9), (0.8, 0.7), (9.0, 2.6))


def boxes(x, y, l, w, yaw):
    """f32 [N, 8, 3], bottom face first (the corner order of the post-process entries)"""
    x, y, l, w, yaw = (np.atleast_1d(np.asarray(v, np.float64)) for v in (x, y, l, w, yaw))
    tx, ty = np.array([1, 1, -1, -1]) * 0.5, np.array([-1, 1, 1, -1]) * 0.5
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    px, py = tx[None] * l[:, None], ty[None] * w[:, None]
    out = np.zeros((len(x), 8, 3), np.float32)
    out[:, :4, 0] = out[:, 4:, 0] = px * c - py * s + x[:, None]
    out[:, :4, 1] = out[:, 4:, 1] = px * s + py * c + y[:, None]
    out[:, :4, 2], out[:, 4:, 2] = -1.0, 0.6
    return out


def _random_frame(g, n_det, n_gt, det_cap, gt_cap):
    """rows past the counts hold plausible boxes too: the kernels must not look at them"""
    r, a, lab = g.uniform(2.0, 108.0, gt_cap), g.uniform(-np.pi, np.pi, gt_cap), g.integers(1, 4, gt_cap)
    gx, gy, gyaw = r * np.cos(a), r * np.sin(a), g.uniform(-np.pi, np.pi, gt_cap)
    gl, gw = np.array(SIZES)[lab - 1].T * g.uniform(0.85, 1.15, (2, gt_cap))
    gt = boxes(gx, gy, gl, gw, gyaw)
    r, a, dlab = g.uniform(2.0, 108.0, det_cap), g.uniform(-np.pi, np.pi, det_cap), g.integers(0, 5, det_cap)     # clutter; labels 0 and 4 belong nowhere
    dx, dy, dyaw = r * np.cos(a), r * np.sin(a), g.uniform(-np.pi, np.pi, det_cap)
    dl, dw = np.array(SIZES)[np.clip(dlab, 1, 3) - 1].T
    if n_gt:
        hit = g.random(det_cap) < 0.8                                 # a jittered copy of a random GT: several detections compete for one
        j = g.integers(0, n_gt, det_cap)
        u = g.uniform(0.0, 1.0, det_cap) ** 2
        dx = np.where(hit, gx[j] + g.normal(0, 1.2, det_cap) * u, dx); dy = np.where(hit, gy[j] + g.normal(0, 1.2, det_cap) * u, dy)
        dyaw = np.where(hit, gyaw[j] + g.normal(0, 0.5, det_cap) * u, dyaw)
        dl = np.where(hit, gl[j] * (1 + g.uniform(-0.3, 0.3, det_cap) * u), dl); dw = np.where(hit, gw[j] * (1 + g.uniform(-0.3, 0.3, det_cap) * u), dw)
        dlab = np.where(hit & (g.random(det_cap) < 0.85), lab[j], dlab)
        if n_det:                                                     # the last GT row always has its detection: an exact copy
            k = n_gt - 1
            dx[0], dy[0], dyaw[0], dl[0], dw[0], dlab[0] = gx[k], gy[k], gyaw[k], gl[k], gw[k], lab[k]
    return boxes(dx, dy, dl, dw, dyaw), dlab.astype(np.int32), gt, lab.astype(np.int32)


def _margins_hold(ref, thresholds, ranges, det, gt):
    bounds = np.array([b for r in ranges for b in r if np.isfinite(b)] or [1e9])
    if ref["iou"].size and np.abs(ref["iou"][..., None] - np.array(thresholds, np.float32)).min() < 1e-4:
        return False
    d = np.concatenate([eval_utils.centre_distance(eval_utils._quads(det)), eval_utils.centre_distance(eval_utils._quads(gt))])
    return not d.size or np.abs(d[:, None] - bounds).min() >= 1e-3


def _reference(case):
    """the CPU path, frame by frame, in the layout of the GPU outputs"""
    F, cap = case["det_corners"].shape[:2]
    nc, thr, rng = case["n_classes"], case["thresholds"], case["ranges"]
    P = max(1, nc) * len(rng) * len(thr)
    out = {"order": np.full((F, cap), -1, np.int32), "scores": np.zeros((F, cap), np.float32), "flags": np.zeros((F, P, cap), np.uint8),
           "match": np.full((F, P, cap), -1, np.int32), "gt": np.zeros((F, P), np.int32), "ok": True}
    for f in range(F):
        n, g = int(case["det_counts"][f]), int(case["gt_counts"][f])
        ref = eval_utils.tp_fp_frame(case["det_corners"][f, :n], case["det_scores"][f, :n], case["gt_corners"][f, :g], thr, rng,
                                     case["det_labels"][f, :n], case["gt_labels"][f, :g], nc)
        out["ok"] &= _margins_hold(ref, thr, rng, case["det_corners"][f, :n], case["gt_corners"][f, :g])
        out["order"][f, :n], out["scores"][f, :n] = ref["order"], ref["scores"]
        out["flags"][f, :, :n], out["match"][f, :, :n], out["gt"][f] = ref["flags"], ref["match"], ref["gt"]
    return out


SHAPES = {
    # name: (det_cap, gt_cap, det counts per frame, GT counts per frame)
    "lanes": (40, 256, (40, 39, 40), (63, 64, 65)),                   # the last lane, a full wave, the first second slot
    "slots": (130, 256, (130, 0, 1), (256, 1, 0)),                    # three chunks of ranks and all four slots; no detection; no GT
    "one_frame": (64, 65, (64,), (65,)),
    "thousand": (1024, 256, (1000,), (200,)),
    "cap_one": (1, 1, (1, 0), (1, 1)),
}


@functools.lru_cache(maxsize=None)
def random_case(shape, n_classes):
    det_cap, gt_cap, dn, gn = SHAPES[shape]
    for seed in range(100, 150):
        g = np.random.default_rng(seed)
        frames = [_random_frame(g, dn[f], gn[f], det_cap, gt_cap) for f in range(len(dn))]
        case = {"det_corners": np.stack([fr[0] for fr in frames]), "det_labels": np.stack([fr[1] for fr in frames]),
                "gt_corners": np.stack([fr[2] for fr in frames]), "gt_labels": np.stack([fr[3] for fr in frames]),
                "det_scores": np.stack([((g.permutation(det_cap) + 1) / (det_cap + 1)).astype(np.float32) for _ in dn]),      # distinct, unsorted
                "det_counts": np.array(dn, np.int32), "gt_counts": np.array(gn, np.int32),
                "n_classes": n_classes, "thresholds": THRESHOLDS, "ranges": RANGES}
        case["ref"] = _reference(case)
        if case["ref"]["ok"]:
            return case
    raise AssertionError("no seed keeps the margins")


def run_gpu(case):
    from quantv2x_amd.evaluation import gpu_tp_fp_batch
    t = {k: torch.from_numpy(case[k]).cuda() for k in ("det_corners", "det_scores", "det_labels", "det_counts", "gt_corners", "gt_labels", "gt_counts")}
    out = gpu_tp_fp_batch(t["det_corners"], t["det_scores"], t["det_labels"], t["det_counts"], t["gt_corners"], t["gt_labels"], t["gt_counts"],
                          thresholds=case["thresholds"], ranges=case["ranges"], num_classes=case["n_classes"])
    return dict(zip(("order", "scores", "flags", "match", "gt"), (o.cpu().numpy() for o in out)))


def assert_same(got, ref):
    for k in ("order", "scores", "gt", "flags", "match"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


@pytest.mark.parametrize("n_classes", [0, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_frames_equal_the_cpu_path(shape, n_classes):
    case = random_case(shape, n_classes)
    ref = case["ref"]
    if shape in ("lanes", "slots", "thousand"):                      # the cases really exercise what they are there for
        assert (ref["flags"] == 2).any() and (ref["flags"] == 1).any() and (ref["flags"][:, :, :] == 0).any()
        for f, (n, g) in enumerate(zip(case["det_counts"], case["gt_counts"])):
            assert not (n and g) or (ref["match"][f] == g - 1).any()  # the last GT row is matched
        assert (ref["gt"][:, 3 * 3:4 * 3] > 0).any()                  # a finite band with GT
    assert_same(run_gpu(case), ref)


def _crafted(det, scores, gt, det_labels=None, gt_labels=None, n_classes=0, thresholds=THRESHOLDS, ranges=RANGES):
    n, g = len(det), len(gt)
    case = {"det_corners": det[None], "det_scores": np.asarray(scores, np.float32)[None],
            "det_labels": np.asarray(det_labels if det_labels is not None else np.ones(n), np.int32)[None],
            "gt_corners": gt[None], "gt_labels": np.asarray(gt_labels if gt_labels is not None else np.ones(g), np.int32)[None],
            "det_counts": np.array([n], np.int32), "gt_counts": np.array([g], np.int32), "n_classes": n_classes,
            "thresholds": thresholds, "ranges": ranges}
    case["ref"] = _reference(case)
    assert case["ref"]["ok"], "a crafted case sits on a margin"
    return case


def test_identical_gt_tie_goes_to_the_lower_row_and_equal_scores_keep_their_rows():
    far = boxes(60.0, 5.0, 4.0, 2.0, 0.3)
    gt = np.concatenate([far, boxes([10.0, 10.0], [0.0, 0.0], 4.0, 2.0, 0.0)])           # rows 1 and 2 identical
    det = np.concatenate([boxes([10.1, 10.2], [0.0, 0.0], 4.0, 2.0, 0.0), far, boxes(80.0, 0.0, 4.0, 2.0, 0.0)])
    case = _crafted(det, [0.8, 0.8, 0.8, 0.9], gt)                    # rows 0, 1, 2 tie: rank order 3, 0, 1, 2
    ref = case["ref"]
    assert ref["order"][0].tolist() == [3, 0, 1, 2]
    assert ref["match"][0, 1].tolist() == [-1, 1, 2, 0] and ref["flags"][0, 1].tolist() == [1, 2, 2, 2]
    assert_same(run_gpu(case), ref)


def test_second_best_gt_above_and_below_the_threshold():
    """the higher-scored detection takes the GT both like best; the other one then matches its second GT where the threshold lets it
    (0.3) and is a false positive where it does not (0.7)"""
    gt = boxes([12.0, 14.4], [0.0, 0.0], 4.0, 2.0, 0.0)
    det = boxes([12.6, 12.1], [0.0, 0.0], 4.0, 2.0, 0.0)              # row 0: IoU 0.74 with GT 0, 0.38 with GT 1; row 1 (higher score): 0.95 with GT 0
    case = _crafted(det, [0.6, 0.9], gt)
    ref = case["ref"]
    assert ref["order"][0].tolist() == [1, 0]
    assert ref["match"][0, 0].tolist() == [0, 1] and ref["flags"][0, 0].tolist() == [2, 2]          # threshold 0.3, all ranges
    assert ref["match"][0, 2].tolist() == [0, -1] and ref["flags"][0, 2].tolist() == [2, 1]         # threshold 0.7
    assert_same(run_gpu(case), ref)


def test_infinite_ranges_an_empty_band_and_foreign_labels():
    gt = boxes([10.0, 60.0, 40.0], [0.0, 0.0, 0.0], 4.0, 2.0, 0.0)
    det = boxes([10.1, 40.2, 10.0, 10.3], [0.0, 0.0, 0.1, 0.0], 4.0, 2.0, 0.0)
    ranges = ((-INF, INF), (-INF, 30.0), (50.0, INF), (30.0, 50.0))   # (50, inf): a GT, no detection
    for n_classes, dl, gl in ((0, [7, 0, -1, 2], [9, 9, 9]), (3, [1, 2, 4, 0], [1, 3, 2])):
        case = _crafted(det, [0.5, 0.9, 0.7, 0.6], gt, dl, gl, n_classes, THRESHOLDS, ranges)
        ref = case["ref"]
        if n_classes == 0:
            assert ref["gt"][0].reshape(4, 3)[:, 0].tolist() == [3, 1, 1, 1] and not ref["flags"][0, 6:9].any()
            assert ref["flags"][0, 1].tolist() == [2, 2, 1, 1]                    # rank order: rows 1, 2, 3, 0; row 2 takes GT 0 from rows 3 and 0
        else:
            assert not ref["flags"][0, :, 1].any() and not ref["flags"][0, :, 2].any()            # labels 4 (rank 1) and 0 (rank 2): in no problem
            assert ref["gt"][0].reshape(3, 4, 3)[:, 0, 0].tolist() == [1, 1, 1]
        assert_same(run_gpu(case), ref)


def test_fixture_through_the_evaluator_gives_the_golden_ap(golden):
    from quantv2x_amd.evaluation import DetectionEvaluator
    fx = golden["eval"]
    out = {k: torch.from_numpy(fx[s]).cuda() for k, s in (("corners", "det_corners"), ("scores", "det_scores"), ("labels", "det_labels"), ("counts", "det_counts"))}
    gt_c, gt_l, gt_n = (torch.from_numpy(fx[k]).cuda() for k in ("gt_corners", "gt_labels", "gt_counts"))
    ev = DetectionEvaluator()
    for s in (slice(0, 2), slice(2, 6)):                              # two updates: the result concatenates them in order
        ev.update({k: v[s] for k, v in out.items()}, gt_c[s], gt_l[s], gt_n[s])
    r = ev.result()
    for ri in range(4):
        for ti in range(3):
            k = f"r{ri}_t{ti}"
            assert abs(r["ap"][0, ri, ti] - float(fx["ap_" + k])) <= 1e-12, k
            np.testing.assert_allclose(r["mrec"][0][ri][ti], fx["mrec_" + k], rtol=0, atol=1e-12)
            np.testing.assert_allclose(r["mpre"][0][ri][ti], fx["mpre_" + k], rtol=0, atol=1e-12)
            assert (r["tp"][0, ri, ti], r["fp"][0, ri, ti], r["gt"][0, ri, ti]) == (int(fx["tp_" + k].sum()), int(fx["fp_" + k].sum()), int(fx["gt_" + k]))
    ev = DetectionEvaluator(ranges=((-INF, INF),), num_classes=3)     # the per-class marks of eval_utils_mc (its AP is taken in append order: not compared)
    ev.update(out, gt_c, gt_l, gt_n)
    r = ev.result()
    for c in (1, 2, 3):
        for ti in range(3):
            k = f"c{c}_t{ti}"
            assert (r["tp"][c - 1, 0, ti], r["fp"][c - 1, 0, ti], r["gt"][c - 1, 0, ti]) == (int(fx["mc_tp_" + k].sum()), int(fx["mc_fp_" + k].sum()), int(fx["mc_gt_" + k]))
    ev.reset()
    assert np.isnan(ev.result()["ap"]).all()


def test_captured_call_replays_on_refreshed_inputs():
    from quantv2x_amd.engine import capture_call
    from quantv2x_amd.evaluation import gpu_tp_fp_batch
    a, b = random_case("lanes", 3), random_case("slots", 3)
    keys = ("det_corners", "det_scores", "det_labels", "det_counts", "gt_corners", "gt_labels", "gt_counts")
    det_cap = max(a["det_corners"].shape[1], b["det_corners"].shape[1])

    def padded(case):                                                 # both cases in one shape: detection rows up to the larger cap
        out = {}
        for k in keys:
            v = case[k]
            if k.startswith("det_") and k != "det_counts":
                pad = np.zeros((v.shape[0], det_cap - v.shape[1]) + v.shape[2:], v.dtype)
                v = np.concatenate([v, pad], axis=1)
            out[k] = v
        return out
    pa, pb = padded(a), padded(b)
    t = {k: torch.from_numpy(pa[k]).cuda() for k in keys}
    replay = capture_call(lambda: gpu_tp_fp_batch(*(t[k] for k in keys), thresholds=THRESHOLDS, ranges=RANGES, num_classes=3))
    for k in keys:
        t[k].copy_(torch.from_numpy(pb[k]).cuda())
    got = [o.cpu().numpy() for o in replay()]
    eager = [o.cpu().numpy() for o in gpu_tp_fp_batch(*(t[k] for k in keys), thresholds=THRESHOLDS, ranges=RANGES, num_classes=3)]
    for g, e in zip(got, eager):
        np.testing.assert_array_equal(g, e)
    n = b["det_corners"].shape[1]
    np.testing.assert_array_equal(got[2][:, :, :n], b["ref"]["flags"])   # and they are the second case's, not the captured one's
    np.testing.assert_array_equal(got[3][:, :, :n], b["ref"]["match"])


def test_plugin_entry_on_gpu_tensors_fills_result_stat_like_the_cpu_path(golden):
    from quantv2x_amd.plugin.utils import eval_utils_mc
    fx = golden["eval"]
    gpu = {t: {"tp": [], "fp": [], "gt": 0, "score": []} for t in (0.5, 0.7)}
    cpu = {t: {"tp": [], "fp": [], "gt": 0, "score": []} for t in (0.5, 0.7)}
    mc_gpu, mc_cpu = {0.5: {"tp": [], "fp": [], "gt": 0}}, {0.5: {"tp": [], "fp": [], "gt": 0}}
    for f in (0, 3):
        n, g = int(fx["det_counts"][f]), int(fx["gt_counts"][f])
        det, sc, gt = fx["det_corners"][f, :n], fx["det_scores"][f, :n][::-1].copy(), fx["gt_corners"][f, :g]      # scores reversed: unsorted input
        for t, (left, right) in ((0.5, (-INF, INF)), (0.7, (30.0, 100.0))):
            eval_utils.caluclate_tp_fp(torch.from_numpy(det).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(gt).cuda(), gpu, t, left, right)
            eval_utils.caluclate_tp_fp(det, sc, gt, cpu, t, left, right)
        eval_utils_mc.caluclate_tp_fp(torch.from_numpy(det).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(gt).cuda(), mc_gpu, 0.5)
        eval_utils_mc.caluclate_tp_fp(det, sc, gt, mc_cpu, 0.5)
    eval_utils.caluclate_tp_fp(None, None, torch.from_numpy(fx["gt_corners"][1, :5]).cuda(), gpu, 0.5)
    eval_utils.caluclate_tp_fp(None, None, fx["gt_corners"][1, :5], cpu, 0.5)
    eval_utils.caluclate_tp_fp(torch.zeros((0, 8, 3)).cuda(), torch.zeros((0,)).cuda(), torch.from_numpy(fx["gt_corners"][1, :5]).cuda(), gpu, 0.7)
    eval_utils.caluclate_tp_fp(np.zeros((0, 8, 3), np.float32), np.zeros((0,), np.float32), fx["gt_corners"][1, :5], cpu, 0.7)
    assert gpu == cpu and mc_gpu == mc_cpu
    assert sum(gpu[0.5]["tp"]) > 10 and sum(gpu[0.7]["fp"]) > 10
