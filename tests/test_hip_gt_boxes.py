"""``qv2x_gt_boxes_f32`` (csrc/gt_boxes.hip) on the GPU against its numpy statement (``gt_boxes_frame``, plugin voxel_postprocessor.py).

Decisions, order, ids, labels, ``counts`` and ``totals`` must be IDENTICAL; corners within one f32 ulp at the coordinate's magnitude ``M``
(``2^-23 M``, ``M`` = the sum of the absolute values of the terms that form it): both sides compute in fp64 and round once, so only a
last-bit difference in ``cos`` / ``sin`` can move the rounding.  The inputs keep the golden fixture's margins (tests/_gt_common.py), and
every output row past a frame's count must still hold the sentinel it was given."""
import numpy as np
import pytest
import torch

from _gt_common import GT_RANGE, by_id_case, by_iou_case, data_dicts, ego_object, golden_case, local_row, pose, statement

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = 12345.0, -7777
ULP = 2.0 ** -23


def run_gpu(case, gt_cap=256, frames=None, agents=None):
    from quantv2x_amd.ground_truth import gpu_gt_boxes_batch
    fs, ag = slice(0, frames), slice(0, agents)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()      # noqa: E731
    boxes = dev(case["boxes"][fs, ag])
    F, width = boxes.shape[0], boxes.shape[3]
    out = {"corners": torch.full((F, gt_cap, 8, 3), SENT_F, dtype=torch.float32, device="cuda"),
           "labels": torch.full((F, gt_cap), SENT_I, dtype=torch.int32, device="cuda") if width == 8 else None,
           "ids": torch.full((F, gt_cap), SENT_I, dtype=torch.int32, device="cuda"),
           "counts": torch.full((F,), SENT_I, dtype=torch.int32, device="cuda"), "totals": torch.full((F,), SENT_I, dtype=torch.int32, device="cuda")}
    got = gpu_gt_boxes_batch(boxes, dev(case["mask"][fs, ag]), dev(case["ids"][fs, ag]) if case["ids"] is not None else None,
                             dev(case["transforms"][fs, ag]), dev(np.minimum(case["agent_counts"][fs], boxes.shape[1])), order=case["order"],
                             mode=case["mode"], gt_range=case["gt_range"], range_xy_only=case["range_xy_only"], gt_cap=gt_cap,
                             iou_threshold=case.get("iou_threshold", 0.05), out=out)
    assert got is out
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in got.items()}


def assert_same(got, want, gt_cap=256):
    assert got["counts"].shape[0] == len(want)
    for f, w in enumerate(want):
        total = len(w["rows"])
        n = min(total, gt_cap)
        assert (int(got["counts"][f]), int(got["totals"][f])) == (n, total), (f, got["counts"][f], got["totals"][f], n, total)
        np.testing.assert_array_equal(got["ids"][f, :n], w["ids"][:n], err_msg=f"frame {f}")
        if w["labels"] is not None:
            np.testing.assert_array_equal(got["labels"][f, :n], w["labels"][:n], err_msg=f"frame {f}")
            assert (got["labels"][f, n:] == SENT_I).all()
        d = np.abs(got["corners"][f, :n].astype(np.float64) - w["corners"][:n])
        assert (d <= ULP * w["M"][:n, None, :]).all(), (f, float(d.max()))
        assert (got["corners"][f, n:] == SENT_F).all() and (got["ids"][f, n:] == SENT_I).all(), f      # rows past the count: untouched


@pytest.fixture(scope="module")
def boundaries():
    # survivors 0, 1, 63, 64, 65 and 256 in one call: the compaction's wave boundaries and the gt_cap edge; frames with different counts
    return by_id_case(11, [(0, 0, 2, 0), (1, 0, 0, 0), (63, 20, 5, 0), (64, 10, 3, 1), (65, 7, 0, 2), (256, 60, 10, 0)], 4, 128)


def test_survivor_counts_at_the_wave_boundaries_and_the_cap(boundaries):
    case, want = boundaries
    assert [len(w["rows"]) for w in want] == [0, 1, 63, 64, 65, 256]
    assert_same(run_gpu(case), want)


def test_a_smaller_cap_cuts_every_frame_in_order(boundaries):
    case, want = boundaries
    got = run_gpu(case, gt_cap=64)
    assert got["counts"].tolist() == [0, 1, 63, 64, 64, 64] and got["totals"].tolist() == [0, 1, 63, 64, 65, 256]
    assert_same(got, want, gt_cap=64)


def test_overflow_is_counted_not_written():
    case, want = by_id_case(12, [(257, 20, 5, 0), (0, 0, 3, 0)], 2, 256)
    got = run_gpu(case)
    assert got["counts"].tolist() == [256, 0] and got["totals"].tolist() == [257, 0]
    assert_same(got, want)                                            # the first 256 in order; the rows behind them (frame 1's) hold the sentinel
    assert (got["corners"][1] == SENT_F).all()


@pytest.mark.parametrize("agents,obj_cap,spec", [(1, 1, (1, 0, 0, 0)), (1, 256, (200, 0, 40, 15)), (1, 256, (180, 0, 60, 16))],
                         ids=["1", "255", "256"])
def test_candidate_counts(agents, obj_cap, spec):
    case, want = by_id_case(13, [spec], agents, obj_cap)
    assert int(case["mask"].sum()) == sum(spec)
    assert_same(run_gpu(case), want)


def test_2048_candidates_every_id_held_by_all_8_agents():
    """8 agents x 256 slots, every slot set; each of 256 ids once per agent, in another slot order per agent: agent 0's copies survive"""
    g = np.random.default_rng(14)
    objs = [ego_object(g, kind) for kind in ["in"] * 200 + ["out"] * 40 + ["zout"] * 16]
    oid = g.choice(2 ** 32, size=256, replace=False).astype(np.int64) - 2 ** 31
    boxes = np.zeros((1, 8, 256, 7), np.float32); ids = np.zeros((1, 8, 256), np.int32); tf = np.zeros((1, 8, 4, 4), np.float32)
    for a in range(8):
        t = pose(g, a == 0)
        tf[0, a] = t
        for s, k in enumerate(g.permutation(256)):
            boxes[0, a, s], ids[0, a, s] = local_row(objs[k], t, "hwl", 7), oid[k]
    case = {"boxes": boxes, "mask": np.ones((1, 8, 256), np.uint8), "ids": ids, "transforms": tf, "agent_counts": np.array([8], np.int32),
            "order": "hwl", "mode": 0, "gt_range": GT_RANGE, "range_xy_only": False}
    want = statement(case)
    assert len(want[0]["rows"]) == 200 and (want[0]["rows"] < 256).all()
    assert_same(run_gpu(case), want)


def test_2048_candidates_all_ids_distinct():
    case, want = by_id_case(15, [(1500, 0, 400, 148)], 8, 256)
    assert int(case["mask"].sum()) == 2048 and len(np.unique(case["ids"])) == 2048
    got = run_gpu(case)
    assert (int(got["counts"][0]), int(got["totals"][0])) == (256, 1500)
    assert_same(got, want)


def test_negative_ids_and_ids_near_int32_max():
    pool = [-2 ** 31, -2 ** 31 + 1, -2, -1, 0, 1, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 - 3, 2 ** 30, -2 ** 30, 65536]
    case, want = by_id_case(16, [(6, 9, 3, 2), (7, 30, 2, 3)], 3, 16, id_pool=pool)
    assert_same(run_gpu(case), want)


def test_agents_past_the_count_and_masked_slots_are_not_looked_at():
    case, want = by_id_case(17, [(12, 10, 6, 2), (30, 25, 5, 0), (0, 0, 0, 0), (40, 40, 9, 3)], 4, 32, used=[1, 2, 0, 4])
    assert case["mask"][0, 1:].all() and case["mask"][2].all()       # set masks and plausible boxes under used ids in the unused agents
    assert_same(run_gpu(case), want)


def test_1_64_and_65_frames():
    g = np.random.default_rng(18)
    spec = [(int(g.integers(0, 12)), int(g.integers(0, 6)), int(g.integers(0, 4)), int(g.integers(0, 3))) for _ in range(65)]
    spec = [(a, b if a else 0, c, d) for a, b, c, d in spec]
    case, want = by_id_case(18, spec, 2, 16, used=[int(g.integers(1, 3)) if sum(s) <= 16 else 2 for s in spec])
    assert_same(run_gpu(case, frames=1), want[:1])
    assert_same(run_gpu(case, frames=64), want[:64])
    assert_same(run_gpu(case), want)                                  # 65: the wrapper's calls of 64


@pytest.mark.parametrize("range_xy_only", [False, True])
@pytest.mark.parametrize("width", [7, 8])
@pytest.mark.parametrize("order", ["hwl", "lwh"])
def test_orders_row_widths_and_the_xy_only_mask(order, width, range_xy_only):
    case, want = by_id_case(19, [(9, 5, 4, 3), (3, 0, 0, 1)], 3, 16, width=width, order=order, range_xy_only=range_xy_only)
    assert [len(w["rows"]) for w in want] == ([12, 4] if range_xy_only else [9, 3])      # the boxes that pass in x and y only
    assert (want[0]["labels"] is not None) == (width == 8)
    assert_same(run_gpu(case), want)


def test_by_iou():
    """one agent; two agents with 0, 64 and 65 vehicle boxes; an infrastructure box overlapping exactly one vehicle box; one overlapping none"""
    case, want = by_iou_case(20, [(20, 0, 0), (0, 0, 12), (64, 30, 20), (65, 40, 25), (12, 1, 0), (12, 0, 1)], 66, used=[1, 2, 2, 2, 2, 2])
    assert [len(w["rows"]) for w in want] == [20, 12, 84, 90, 12, 13]
    assert_same(run_gpu(case), want)
    assert_same(run_gpu(case, frames=1, agents=1), want[:1])          # and with one agent in the descriptor
    case["order"] = "lwh"
    case["boxes"] = np.ascontiguousarray(case["boxes"][..., [0, 1, 2, 5, 4, 3, 6]])
    assert_same(run_gpu(case), want)


@pytest.mark.parametrize("which", ["single", "mc", "iou"])
def test_golden_frames_against_the_reference(golden, which):
    """the fixture on the GPU against the reference's own results directly (bound: the CPU suite's 32 u M)"""
    fx = golden["gt_boxes"]
    case = golden_case(fx, which)
    want = statement(case)
    got = run_gpu(case)
    assert_same(got, want)
    for f in range(6):
        n = int(fx[f"ref_{which}_counts"][f])
        assert int(got["counts"][f]) == n == int(got["totals"][f])
        key = fx["ref_iou_rows" if which == "iou" else f"ref_{which}_ids"][f, :n]
        assert sorted(got["ids"][f, :n].tolist()) == sorted(key.tolist())
        back = {int(v): k for k, v in enumerate(key)}
        idx = [back[int(v)] for v in got["ids"][f, :n]]
        d = np.abs(got["corners"][f, :n].astype(np.float64) - fx[f"ref_{which}_corners"][f, :n][idx])
        assert (d <= 32 * 2.0 ** -24 * want[f]["M"][:, None, :]).all(), f
        if which == "mc":
            assert got["labels"][f, :n].tolist() == fx["ref_mc_labels"][f, :n][idx].tolist()


def _postprocessors(fx):
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor_3heads import VoxelPostprocessor3Heads
    single = VoxelPostprocessor.__new__(VoxelPostprocessor)
    single.params = {"order": "hwl", "gt_range": fx["gt_range"].tolist()}
    mc = VoxelPostprocessor3Heads.__new__(VoxelPostprocessor3Heads)
    mc.order, mc.gt_range = "hwl", fx["gt_range_mc"].tolist()
    return single, mc


def test_assembler_captured_in_a_graph_replays_on_refilled_buffers(golden):
    from quantv2x_amd.engine import capture_call
    from quantv2x_amd.ground_truth import GroundTruthAssembler
    fx = golden["gt_boxes"]
    post = _postprocessors(fx)[1]
    case = golden_case(fx, "mc")
    dicts = data_dicts(case, "transformation_matrix")
    asm = GroundTruthAssembler(post, max_agents=5, obj_cap=60, gt_cap=256, frames=4)
    asm.fill(dicts[:4])
    replay = capture_call(asm)
    first = {k: v.cpu().numpy() for k, v in replay().items()}
    assert first["counts"].tolist() == fx["ref_mc_counts"][:4].tolist()
    asm.fill([dicts[5], dicts[2], dicts[4]])                          # another frame set, in place; the fourth frame becomes empty
    got = {k: v.cpu().numpy().copy() for k, v in replay().items()}
    eager = GroundTruthAssembler(post, max_agents=5, obj_cap=60, gt_cap=256, frames=4).fill([dicts[5], dicts[2], dicts[4]])()
    want = statement(case)
    assert got["counts"].tolist() == [len(want[5]["rows"]), len(want[2]["rows"]), 0, 0] == got["totals"].tolist()
    for k, v in eager.items():
        e = v.cpu().numpy()
        for f in range(4):
            n = int(got["counts"][f])
            np.testing.assert_array_equal(got[k][f][:n] if got[k].ndim > 1 else got[k][f], e[f][:n] if e.ndim > 1 else e[f], err_msg=k)
    np.testing.assert_array_equal(got["ids"][0, :got["counts"][0]], want[5]["ids"])


def test_reference_named_methods_on_reference_shaped_data_dicts(golden):
    fx = golden["gt_boxes"]
    single, mc = _postprocessors(fx)
    case = golden_case(fx, "single")
    want = statement(case)
    for f, d in enumerate(data_dicts(case, "transformation_matrix_clean")):
        got = single.generate_gt_bbx(d)
        assert got.is_cuda and tuple(got.shape) == (len(want[f]["rows"]), 8, 3) and got.dtype == torch.float32
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want[f]["corners"]) <= ULP * want[f]["M"][:, None, :]).all()
    case = golden_case(fx, "mc")
    want = statement(case)
    for f, d in enumerate(data_dicts(case, "transformation_matrix", as_torch=True)):
        boxes, labels = mc.generate_gt_bbx(d)
        assert tuple(boxes.shape) == (len(want[f]["rows"]), 8, 3) and labels.dtype == torch.float32
        assert labels.cpu().numpy().tolist() == want[f]["labels"].tolist()
        assert (np.abs(boxes.cpu().numpy().astype(np.float64) - want[f]["corners"]) <= ULP * want[f]["M"][:, None, :]).all()
    case = golden_case(fx, "iou")
    want = statement(case)
    for f, d in enumerate(data_dicts(case, "transformation_matrix_clean", as_torch=False)):      # numpy members too
        got = single.generate_gt_bbx_by_iou(d)
        assert tuple(got.shape) == (len(want[f]["rows"]), 8, 3)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want[f]["corners"]) <= ULP * want[f]["M"][:, None, :]).all()


def test_evaluator_update_from_equals_update_on_the_statement(golden):
    """end to end: assembler output into ``update_from`` against ``update`` on the numpy statement's padded arrays"""
    from quantv2x_amd.evaluation import DetectionEvaluator
    from quantv2x_amd.ground_truth import GroundTruthAssembler
    fx = golden["gt_boxes"]
    case = golden_case(fx, "mc")
    want = statement(case)
    g = np.random.default_rng(21)
    F, det_cap = 6, 64
    det = np.zeros((F, det_cap, 8, 3), np.float32); sc = np.zeros((F, det_cap), np.float32); lab = np.zeros((F, det_cap), np.int32); dn = np.zeros((F,), np.int32)
    gt_c = np.zeros((F, 256, 8, 3), np.float32); gt_l = np.zeros((F, 256), np.int32); gt_n = np.zeros((F,), np.int32)
    for f, w in enumerate(want):
        n = len(w["rows"])
        gt_c[f, :n], gt_l[f, :n], gt_n[f] = w["corners"], w["labels"], n
        k = min(n, det_cap)
        dn[f] = k
        shift = np.zeros((k, 1, 3), np.float32)
        shift[:, 0, :2] = g.choice([0.05, 0.4, 0.9, 3.0], size=(k, 1)) * g.choice([-1.0, 1.0], size=(k, 2))     # IoUs well off the thresholds
        det[f, :k], lab[f, :k] = w["corners"][:k] + shift, w["labels"][:k]
        sc[f, :k] = np.sort(g.permutation(1000)[:k].astype(np.float32) / 1000.0)[::-1]
    out = {"corners": torch.from_numpy(det).cuda(), "scores": torch.from_numpy(sc).cuda(), "labels": torch.from_numpy(lab).cuda(), "counts": torch.from_numpy(dn).cuda()}
    asm = GroundTruthAssembler(_postprocessors(fx)[1], max_agents=5, obj_cap=60, gt_cap=256, frames=6).fill(data_dicts(case, "transformation_matrix"))
    a, b = DetectionEvaluator(num_classes=3), DetectionEvaluator(num_classes=3)
    a.update_from(out, asm())
    b.update(out, torch.from_numpy(gt_c).cuda(), torch.from_numpy(gt_l).cuda(), torch.from_numpy(gt_n).cuda())
    ra, rb = a.result(), b.result()
    assert int(ra["tp"].sum()) > 50 and int(ra["fp"].sum()) > 10
    for k in ("ap", "tp", "fp", "gt"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert ra["mrec"] == rb["mrec"] and ra["mpre"] == rb["mpre"]
