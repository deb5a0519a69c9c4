"""``PointsToBoxes`` (sweeps -> pillars -> model -> boxes, three calls for the whole batch) against the chain of the per-frame entries:
``GpuVoxelizer.fixed``, the engine, one ``gpu_post_process`` per frame -- the same boxes, scores and labels, bit for bit, eagerly and
from a replayed HIP graph.  Tiny model.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from quantv2x_amd import synth

pytestmark = pytest.mark.gpu
CAP, FRAMES, POINTS, MAX_BOXES = 1024, 3, 2400, 200


@pytest.fixture(scope="module")
def chain():
    from _common import calibrated_plugin
    from quantv2x_amd.engine import deploy
    from quantv2x_amd.pipeline import PointsToBoxes
    from quantv2x_amd.plugin.data_utils.post_processor import build_postprocessor
    from quantv2x_amd.ptq_state import export_ptq_state
    from quantv2x_amd.voxelizer import GpuVoxelizer
    lidar, vox = synth.SHAPES["tiny"][0], synth.SHAPES["tiny"][1]
    gw, gh, _ = synth.grid_size(lidar, vox)
    eng = deploy(state=export_ptq_state(calibrated_plugin()))
    vz = GpuVoxelizer(lidar, vox, 32, 2048)
    pp = build_postprocessor(synth.mc_postprocess_params(lidar, gw, gh), train=False)
    return PointsToBoxes(eng, vz, pp, CAP, max_boxes=MAX_BOXES)


def _clouds(k):
    lidar = synth.SHAPES["tiny"][0]
    cs = [synth.make_points(lidar, 3000, 70 + FRAMES * k + f, 6.0)[:POINTS].copy() for f in range(FRAMES)]      # (a graph fixes the point count)
    assert all(c.shape[0] == POINTS for c in cs)
    return cs


def _per_frame(p2b, sweeps):
    """the chain as bench.points_to_boxes_line builds it: ``fixed`` (one C call per sweep), the engine, one post-process call per frame"""
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gpu_post_process
    frames = len(sweeps)
    pp = p2b.postprocessor
    pairwise = torch.eye(4, dtype=torch.float64).reshape(1, 1, 1, 4, 4).repeat(frames, 5, 5, 1, 1).cuda()
    inp = p2b.voxelizer.fixed(sweeps, CAP)
    o = p2b.engine({"inputs_m1": inp, "agent_modality_list": ["m1"] * frames, "record_len": torch.ones(frames, dtype=torch.int64),
                    "pairwise_t_matrix": pairwise})
    res = []
    for f in range(frames):
        res.append(gpu_post_process(pp, o["cls_preds"][f:f + 1], o["reg_preds"][f:f + 1], None, p2b.anchors_dev, torch.eye(4),
                                    anchors_per_cell=p2b.per_cell, num_classes=int(o["cls_preds"].shape[1] // p2b.per_cell), num_bins=0,
                                    dir_offset=0.0, rng=pp.gt_range, range_xy_only=True, max_extent=100.0, z_lim=(-100.0, 100.0),
                                    max_boxes=MAX_BOXES, sync=False))
    torch.cuda.synchronize()
    return inp, [tuple(t.clone() for t in r) for r in res]


def _assert_same(out, want_inp, want):
    torch.cuda.synchronize()
    assert torch.equal(out["voxel_counts"], want_inp["voxel_counts"])
    total = 0
    for f, (corners, scores, labels, count) in enumerate(want):
        k = int(count)
        assert int(out["counts"][f]) == k, f
        assert torch.equal(out["corners"][f, :k], corners[:k]) and torch.equal(out["scores"][f, :k], scores[:k]), f
        assert torch.equal(out["labels"][f, :k], labels[:k]), f
        total += k
    return total


def test_three_frames_equal_the_per_frame_chain(chain):
    sweeps = [torch.from_numpy(c).cuda() for c in _clouds(0)]
    out = chain(sweeps)
    assert out["corners"].shape == (FRAMES, MAX_BOXES, 8, 3) and out["counts"].shape == (FRAMES,)
    assert _assert_same(out, *_per_frame(chain, sweeps)) > 0             # the frames do end in boxes
    assert (out["voxel_counts"] > 100).all()


def test_captured_chain_replays_on_new_sweeps(chain):
    sets = [_clouds(k) for k in (0, 1, 2)]
    sweeps = [torch.from_numpy(c).cuda() for c in sets[0]]
    replay = chain.capture(sweeps)
    seen = []
    for k in (1, 2):
        for s, c in zip(sweeps, sets[k]):
            s.copy_(torch.from_numpy(c))
        out = replay()
        torch.cuda.synchronize()
        got = {key: v.clone() for key, v in out.items()}
        assert _assert_same(got, *_per_frame(chain, [torch.from_numpy(c).cuda() for c in sets[k]])) > 0
        seen.append(got["voxel_counts"].tolist())
    assert seen[0] != seen[1]
