"""``PointsToBoxes`` with the single-class ``VoxelPostprocessor`` (the post-processor of the OPV2V and DAIR-V2X yamls): the boxes of a batch
equal one ``gpu_post_process`` per frame with the parameters ``VoxelPostprocessor.post_process`` uses -- one class, the direction head's
bins and offset from ``dir_args``, the full range mask, ``max_extent`` 6, z in [-3, 1] -- bit for bit, eagerly and from a replayed HIP
graph; a model without a direction head is post-processed without one, as the class does.  Tiny single-class model.  Needs an MI355X."""
import pytest
import torch

from quantv2x_amd import synth

pytestmark = pytest.mark.gpu
CAP, FRAMES, POINTS, MAX_BOXES = 1024, 2, 2400, 200
LIDAR, VOX = synth.SHAPES["tiny"][0], synth.SHAPES["tiny"][1]
SEED = 70                                        # (both frames of the sets used below end in boxes)
DIR_ARGS = {"dir_offset": 0.7853, "num_bins": 2, "anchor_yaw": [0, 90]}


def _params(gw, gh):
    return {"core_method": "VoxelPostprocessor", "gt_range": list(LIDAR), "order": "hwl", "max_num": 100, "nms_thresh": 0.15,
            "anchor_args": {"cav_lidar_range": list(LIDAR), "l": 3.9, "w": 1.6, "h": 1.56, "r": [0, 90], "feature_stride": 2, "num": 2,
                            "vw": VOX[0], "vh": VOX[1], "vd": VOX[2], "W": gw, "H": gh, "D": 1},
            "target_args": {"score_threshold": 0.2}, "dir_args": dict(DIR_ARGS)}


@pytest.fixture(scope="module")
def chain():
    from _common import calibrated_plugin
    from quantv2x_amd.engine import deploy
    from quantv2x_amd.pipeline import PointsToBoxes
    from quantv2x_amd.plugin.data_utils.post_processor import build_postprocessor
    from quantv2x_amd.ptq_state import export_ptq_state
    from quantv2x_amd.voxelizer import GpuVoxelizer
    gw, gh, _ = synth.grid_size(LIDAR, VOX)
    eng = deploy(state=export_ptq_state(calibrated_plugin(multiclass=False)))
    p2b = PointsToBoxes(eng, GpuVoxelizer(LIDAR, VOX, 32, 2048), build_postprocessor(_params(gw, gh), train=False), CAP, max_boxes=MAX_BOXES)
    assert p2b.per_cell == 2 and tuple(p2b.anchors_dev.shape) == ((gh // 2) * (gw // 2) * 2, 7)
    return p2b


def _clouds(k):
    cs = [synth.make_points(LIDAR, 3000, SEED + FRAMES * k + f, 6.0)[:POINTS].copy() for f in range(FRAMES)]     # (a graph fixes the point count)
    assert all(c.shape[0] == POINTS for c in cs)
    return cs


def _dev(clouds):
    return [torch.from_numpy(c).cuda() for c in clouds]


class _Spy:
    """records what the engine of a ``PointsToBoxes`` returns, after ``edit`` had its way with it"""

    def __init__(self, p2b, edit=lambda o: o):
        self.p2b, self.engine, self.edit, self.outs = p2b, p2b.engine, edit, []

    def __enter__(self):
        self.p2b.engine = lambda d: self.outs.append(self.edit(self.engine(d))) or self.outs[-1]
        return self

    def __exit__(self, *exc):
        self.p2b.engine = self.engine


def _per_frame(p2b, o, with_dir):
    """one ``gpu_post_process`` per frame on the head maps ``o`` with the class's own parameters"""
    from quantv2x_amd.plugin.data_utils.post_processor.voxel_postprocessor import gpu_post_process
    pp = p2b.postprocessor
    res = []
    for f in range(o["cls_preds"].shape[0]):
        res.append(gpu_post_process(pp, o["cls_preds"][f:f + 1], o["reg_preds"][f:f + 1], o["dir_preds"][f:f + 1] if with_dir else None,
                                    p2b.anchors_dev, torch.eye(4), anchors_per_cell=2, num_classes=1, num_bins=DIR_ARGS["num_bins"] if with_dir else 0,
                                    dir_offset=DIR_ARGS["dir_offset"] if with_dir else 0.0, rng=pp.params["gt_range"], range_xy_only=False,
                                    max_extent=6.0, z_lim=(-3.0, 1.0), max_boxes=MAX_BOXES, sync=False))
    torch.cuda.synchronize()
    return [tuple(t.clone() for t in r) for r in res]


def _assert_same(out, want):
    """-> the box count per frame"""
    torch.cuda.synchronize()
    assert out["counts"].shape == (len(want),) and out["corners"].shape == (len(want), MAX_BOXES, 8, 3)
    ks = []
    for f, (corners, scores, labels, count) in enumerate(want):
        k = int(count)
        print("frame", f, "boxes", k)
        assert int(out["counts"][f]) == k, f
        assert torch.equal(out["corners"][f, :k], corners[:k]) and torch.equal(out["scores"][f, :k], scores[:k]), f
        assert torch.equal(out["labels"][f, :k], labels[:k]), f
        ks.append(k)
    return ks


def test_two_frames_equal_the_per_frame_post_process_with_the_direction_head(chain):
    with _Spy(chain) as spy:
        out = chain(_dev(_clouds(0)))
    torch.cuda.synchronize()
    o = spy.outs[0]
    assert o["cls_preds"].shape[1] == 2 and o["dir_preds"].shape[1] == 4            # one class x two anchors; two bins per anchor
    ks = _assert_same(out, _per_frame(chain, o, with_dir=True))
    assert all(k > 0 for k in ks), ks                                               # the comparison is about boxes, not about empty frames
    assert (out["labels"][0, :ks[0]] == out["labels"][0, 0]).all()                  # one class
    # the direction head took part: the same maps without it give other corners somewhere
    flat = _per_frame(chain, o, with_dir=False)
    assert any(int(c[3]) != k or not torch.equal(c[0][:k], out["corners"][f, :k]) for f, (c, k) in enumerate(zip(flat, ks)))


def test_a_model_without_a_direction_head_is_post_processed_without_one(chain):
    """``VoxelPostprocessor.post_process`` decides by the outputs (``dir_preds`` present or not), not by the yaml's ``dir_args``"""
    with _Spy(chain, edit=lambda o: {k: v for k, v in o.items() if k != "dir_preds"}) as spy:
        out = chain(_dev(_clouds(0)))
    torch.cuda.synchronize()
    ks = _assert_same(out, _per_frame(chain, spy.outs[0], with_dir=False))
    assert any(k > 0 for k in ks), ks


def test_captured_chain_replays_on_new_sweeps(chain):
    sets = [_clouds(k) for k in (0, 1)]
    sweeps = _dev(sets[0])
    replay = chain.capture(sweeps)
    for s, c in zip(sweeps, sets[1]):
        s.copy_(torch.from_numpy(c))
    out = replay()
    torch.cuda.synchronize()
    got = {key: v.clone() for key, v in out.items()}
    with _Spy(chain) as spy:
        chain(_dev(sets[1]))
    torch.cuda.synchronize()
    ks = _assert_same(got, _per_frame(chain, spy.outs[0], with_dir=True))
    assert any(k > 0 for k in ks), ks
