"""Ground-truth boxes without a GPU: the numpy statement of ``qv2x_gt_boxes_f32`` (``gt_boxes_frame`` in the plugin's
``voxel_postprocessor.py``) against what the reference's own ``generate_gt_bbx`` / ``generate_gt_bbx_by_iou`` gave on
tests/golden/gt_boxes.npz (tests/golden/make_golden_gt.py), the first-occurrence rule, the assembler's host side and the C entry's
argument checks.

Corner tolerance (derived, not measured): the reference chains about ten fp32 roundings -- the half extents, two products and a sum per
rotated coordinate, the centre, three products and three sums in the 4x4 transform -- on quantities bounded by ``M``, the sum of the absolute
values of the terms that form the coordinate, plus ``sinf`` / ``cosf`` to a few ulp: ``16 u M`` with ``u = 2^-24``, doubled for slack.  The
statement computes in fp64 and rounds once (``u M``), inside that.  At the fixture's magnitudes the bound stays below 1e-3 m, inside the
2e-3 m margin every mask decision of the fixture keeps."""
import ctypes as C
import math

import numpy as np
import pytest

from _gt_common import by_id_case, by_iou_case, data_dicts, golden_case, statement

U = 2.0 ** -24


@pytest.fixture(scope="module")
def fx(golden):
    return golden["gt_boxes"]


@pytest.mark.parametrize("which", ["single", "mc"])
def test_statement_reproduces_the_reference_by_id(fx, which):
    want = statement(golden_case(fx, which))
    for f, got in enumerate(want):
        n = int(fx[f"ref_{which}_counts"][f])
        ref_ids, ref_c = fx[f"ref_{which}_ids"][f, :n], fx[f"ref_{which}_corners"][f, :n]
        assert len(got["ids"]) == n and len(set(ref_ids.tolist())) == n, f
        assert set(got["ids"].tolist()) == set(ref_ids.tolist()), f
        back = {int(v): k for k, v in enumerate(ref_ids)}
        idx = [back[int(v)] for v in got["ids"]]
        if which == "mc":
            assert got["labels"].tolist() == fx["ref_mc_labels"][f, :n][idx].tolist() and set(got["labels"].tolist()) <= {1, 2, 3}, f
        else:
            assert got["labels"] is None
        bound = 32 * U * got["M"]
        print(which, "frame", f, "boxes", n, "max |diff|", float(np.abs(got["corners"] - ref_c[idx]).max()) if n else 0.0, "max bound", float(bound.max()) if n else 0.0)
        assert n == 0 or bound.max() < 1e-3
        assert (np.abs(got["corners"].astype(np.float64) - ref_c[idx]) <= bound[:, None, :]).all(), f
        assert (np.diff(got["rows"]) > 0).all()                      # candidate order


def test_statement_reproduces_the_reference_by_iou(fx):
    want = statement(golden_case(fx, "iou"))
    dropped = 0
    for f, got in enumerate(want):
        n = int(fx["ref_iou_counts"][f])
        assert got["rows"].tolist() == fx["ref_iou_rows"][f, :n].tolist(), f      # the reference keeps concatenation order here: rows in order
        bound = 32 * U * got["M"]
        assert (np.abs(got["corners"].astype(np.float64) - fx["ref_iou_corners"][f, :n]) <= bound[:, None, :]).all(), f
        dropped += int(fx["iou_mask"][f, :int(fx["iou_agent_counts"][f])].sum()) - n
    assert dropped > 30                                               # the fixture does drop boxes (IoU filter and range mask)


def test_first_occurrence_rule_on_the_differing_copies(fx):
    """one id, two different boxes, one in range and one out of range: only the FIRST occurrence's box is range-masked"""
    want = statement(golden_case(fx, "single"))
    out_first, in_first = (int(v) for v in fx["special_ids"])
    for f, oid in ((1, out_first), (2, in_first)):                   # both copies are candidates
        assert ((fx["ids"][f, :2] == oid) & (fx["mask"][f, :2] == 1)).sum(axis=1).tolist() == [1, 1]
    assert out_first not in want[1]["ids"].tolist() and out_first not in fx["ref_single_ids"][1].tolist()
    assert in_first in want[2]["ids"].tolist() and in_first in fx["ref_single_ids"][2].tolist()
    k = want[2]["ids"].tolist().index(in_first)
    assert want[2]["rows"][k] < fx["boxes"].shape[2]                  # agent 0's copy
    # and on two boxes built here, in both orders
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gt_boxes_frame
    inside, outside = [10, 5, -1, 1.6, 1.9, 4.2, 0.3], [10, 60, -1, 1.6, 1.9, 4.2, 0.3]
    tf = np.stack([np.eye(4, dtype=np.float32)] * 2)
    for first, second, n in ((outside, inside, 0), (inside, outside, 1)):
        r = gt_boxes_frame(np.array([[first], [second]], np.float32), np.ones((2, 1)), np.array([[5], [5]]), tf, order="hwl", mode=0,
                           gt_range=[-140, -40, -3, 140, 40, 1], range_xy_only=False)
        assert len(r["rows"]) == n and r["rows"].tolist() == [0][:n]
    r = gt_boxes_frame(np.array([[outside], [inside]], np.float32), np.ones((2, 1)), np.array([[5], [6]]), tf, order="hwl", mode=0,
                       gt_range=[-140, -40, -3, 140, 40, 1], range_xy_only=False)
    assert r["rows"].tolist() == [1] and r["ids"].tolist() == [6]


def test_corner_order_and_the_column_permutation():
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gt_project_boxes
    c = gt_project_boxes(np.array([[1, 2, 3, 2.0, 4.0, 6.0, 0.0]], np.float32), np.eye(4), "hwl")[0]      # h 2, w 4, l 6
    assert c.tolist() == [[4, 0, 2], [4, 4, 2], [-2, 4, 2], [-2, 0, 2], [4, 0, 4], [4, 4, 4], [-2, 4, 4], [-2, 0, 4]]
    c = gt_project_boxes(np.array([[1, 2, 3, 6.0, 4.0, 2.0, 0.0]], np.float32), np.eye(4), "lwh")[0]
    assert c[0].tolist() == [4, 0, 2] and c[6].tolist() == [-2, 4, 4]
    t = np.eye(4); t[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]; t[:3, 3] = [10, 20, 30]                # a quarter turn and a shift
    c = gt_project_boxes(np.array([[1, 2, 3, 2.0, 4.0, 6.0, 0.0]], np.float32), t, "hwl")[0]
    assert c[0].tolist() == [10, 24, 32]


def test_synthetic_cases_are_what_their_spec_says():
    """the generators the GPU suite uses, on the CPU: survivor counts by construction, both modes, decoys never looked at"""
    case, want = by_id_case(3, [(5, 4, 3, 2), (0, 0, 2, 0), (1, 0, 0, 0)], 3, 8, width=8, used=[3, 2, 1])
    assert [len(w["rows"]) for w in want] == [5, 0, 1] and want[0]["labels"].dtype == np.int32
    case["range_xy_only"] = True
    assert [len(w["rows"]) for w in statement(case)] == [7, 0, 1]
    case, want = by_iou_case(4, [(6, 3, 4), (5, 2, 2), (0, 0, 3)], 8, used=[2, 1, 2])
    assert [len(w["rows"]) for w in want] == [10, 5, 3]


def test_assembler_scatters_ids_into_the_mask_slots(fx):
    from quantv2x_amd.ground_truth import GroundTruthAssembler
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor_3heads import VoxelPostprocessor3Heads
    post = VoxelPostprocessor.__new__(VoxelPostprocessor)
    post.params = {"order": "hwl", "gt_range": fx["gt_range"].tolist()}
    case = golden_case(fx, "single")
    asm = GroundTruthAssembler(post, max_agents=5, obj_cap=60, gt_cap=256, frames=8, device="cpu")
    boxes, mask, ids, tf, counts = asm.host_arrays(data_dicts(case, "transformation_matrix_clean"))
    assert counts.tolist() == case["agent_counts"].tolist() + [0, 0] and not mask[6:].any()
    for f in range(6):
        n = int(counts[f])
        np.testing.assert_array_equal(boxes[f, :n], case["boxes"][f, :n])
        np.testing.assert_array_equal(mask[f, :n], case["mask"][f, :n])
        np.testing.assert_array_equal(tf[f, :n], case["transforms"][f, :n])
        m = mask[f, :n] == 1
        np.testing.assert_array_equal(ids[f, :n][m], case["ids"][f, :n][m])
        assert not mask[f, n:].any()
    assert (asm.mode, asm.row_floats, asm.transform_key, asm.range_xy_only) == (0, 7, "transformation_matrix_clean", False)
    with pytest.raises(ValueError, match="GPU"):
        asm.fill(data_dicts(case, "transformation_matrix_clean"))()
    by_iou = GroundTruthAssembler(post, max_agents=2, obj_cap=60, gt_cap=256, by_iou=True, device="cpu")
    assert (by_iou.mode, by_iou.range_xy_only) == (1, True)
    mc = VoxelPostprocessor3Heads.__new__(VoxelPostprocessor3Heads)
    mc.order, mc.gt_range = "hwl", fx["gt_range_mc"].tolist()
    asm = GroundTruthAssembler(mc, max_agents=5, obj_cap=60, gt_cap=256, frames=6, device="cpu")
    assert (asm.mode, asm.row_floats, asm.transform_key, asm.range_xy_only) == (0, 8, "transformation_matrix", True)
    boxes = asm.host_arrays(data_dicts(golden_case(fx, "mc"), "transformation_matrix", as_torch=False))[0]
    np.testing.assert_array_equal(boxes[0], fx["boxes"][0])
    bad = data_dicts(case, "transformation_matrix_clean")[:1]
    bad[0]["cav0"]["object_ids"] = bad[0]["cav0"]["object_ids"][:-1]
    with pytest.raises(ValueError, match="object_ids"):
        GroundTruthAssembler(post, 5, 60, 256, device="cpu").host_arrays(bad)
    for kw in (dict(max_agents=9), dict(obj_cap=257), dict(gt_cap=257), dict(max_agents=3, by_iou=True)):
        with pytest.raises(ValueError):
            GroundTruthAssembler(post, **{**dict(max_agents=2, obj_cap=8, gt_cap=8, device="cpu"), **kw})


def test_argument_errors_of_the_gt_entry_without_gpu():
    from quantv2x_amd import build, lib
    build.build()
    l = lib.load()
    assert C.sizeof(lib.GtDesc) == 8 * 4 + 6 * 4 + 4

    def desc(**kw):
        d = lib.GtDesc()
        d.frames, d.agents, d.obj_cap, d.gt_cap, d.row_floats, d.order, d.mode, d.range_xy_only = 2, 2, 16, 40, 7, 0, 0, 0
        for i, v in enumerate([-140, -40, -3, 140, 40, 1]):
            d.range[i] = v
        d.iou_threshold = 0.05
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)

    def call(d, args=None):
        return l.qv2x_gt_boxes_f32(C.byref(d) if d is not None else None, *([p] * 10 if args is None else args), None)
    assert call(None) == -1 and b"descriptor" in l.qv2x_last_error()
    for bad in (dict(frames=0), dict(frames=65), dict(agents=0), dict(agents=9), dict(obj_cap=0), dict(obj_cap=257), dict(gt_cap=0), dict(gt_cap=257),
                dict(row_floats=6), dict(row_floats=9), dict(order=-1), dict(order=2), dict(mode=-1), dict(mode=2), dict(range_xy_only=2),
                dict(mode=1, agents=3)):
        assert call(desc(**bad)) == -1, bad
        word = {"range_xy_only": "range_xy_only", "row_floats": "row_floats", "obj_cap": "obj_cap", "gt_cap": "gt_cap"}.get(next(iter(bad)), next(iter(bad)).rstrip("s"))
        assert word in l.qv2x_last_error().decode(), (bad, l.qv2x_last_error())
    d = desc()
    d.range[4] = math.nan
    assert call(d) == -1 and b"range" in l.qv2x_last_error()
    for thr in (-0.1, 1.5, math.nan):
        assert call(desc(mode=1, iou_threshold=thr)) == -1 and b"iou_threshold" in l.qv2x_last_error()
    for i in (0, 1, 3, 4, 5, 8, 9):                                   # boxes, mask, transforms, agent_counts, gt_corners, gt_counts, gt_totals
        a = [p] * 10
        a[i] = None
        assert call(desc(), a) == -1 and b"null" in l.qv2x_last_error(), i
    a = [p] * 10
    a[2] = None                                                       # ids: optional only in mode 1
    assert call(desc(), a) == -1 and b"ids" in l.qv2x_last_error()
    a = [p] * 10
    a[6] = None                                                       # gt_labels: optional only for 7-float rows
    assert call(desc(row_floats=8), a) == -1 and b"gt_labels" in l.qv2x_last_error()
