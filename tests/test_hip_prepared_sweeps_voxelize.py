"""The sentinel form of ``plugin.utils.pcd_utils.prepare_sweep`` through the GPU voxelizer: a sweep whose removed points are ``(qNaN, qNaN,
qNaN, 0)`` rows gives the pillars of the host-compacted sweep (the removed rows deleted) -- features, coords, counts and ``voxel_counts``
equal, so no sentinel reaches a pillar and the first-come order survives -- from ``fixed_batch`` and from ``fixed``.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from quantv2x_amd import synth

pytestmark = pytest.mark.gpu
CAP = 1024


@pytest.mark.parametrize("with_transform", [False, True])
def test_prepared_sweeps_give_the_pillars_of_the_compacted_sweeps(with_transform):
    from quantv2x_amd.plugin.utils.pcd_utils import kept_rows, prepare_sweep
    from quantv2x_amd.voxelizer import GpuVoxelizer
    lidar, vox = synth.SHAPES["tiny"][0], synth.SHAPES["tiny"][1]
    vz = GpuVoxelizer(lidar, vox, 32, 2048)
    sweeps = [synth.make_points(lidar, n, 90 + k, 4.0) for k, n in enumerate((3000, 1500, 2200))]
    sweeps[1][::50, 1] = np.nan                                       # NaN padding rows in between
    tf = [synth.pose_matrix(1.5 * k, -0.5 * k, 0.2 * k) if with_transform else None for k in range(3)]
    prepared = [prepare_sweep(s, tf[k], True) for k, s in enumerate(sweeps)]
    compact = [kept_rows(p) for p in prepared]
    assert all(p.shape == s.shape and 0 < c.shape[0] < s.shape[0] - 100 for p, c, s in zip(prepared, compact, sweeps))
    up = lambda arrays: [torch.from_numpy(a).cuda() for a in arrays]      # noqa: E731
    for run in (lambda a: vz.fixed_batch(up(a), CAP), lambda a: vz.fixed(up(a), CAP)):
        got, want = run(prepared), run(compact)
        torch.cuda.synchronize()
        for k in ("voxel_counts", "voxel_coords", "voxel_num_points", "voxel_features"):
            assert torch.equal(got[k], want[k]), k
        assert (got["voxel_counts"] > 100).all() and not torch.isnan(got["voxel_features"]).any()
