"""``qv2x_lss_plan_f32`` / ``qv2x_lss_splat_f32`` (csrc/lift_splat.hip) behind ``GpuLiftSplat`` on the GPU: the three scenes of
tests/golden/lift_splat.npz (the reference's own ``get_geometry`` + ``voxel_pooling``) and constructed cases, each the smallest shape that
reaches its path.  Cells must EQUAL ``cells_statement(geometry_statement(...))``; every output element must lie within the derived fp32
bound of ``splat_statement``: ``(n + 2) * 2^-24 * S`` plus the underflow floor, with ``n`` the cell's points and
``S`` the float64 sum of ``|p * f|`` over it.  Largest measured ratio to the bound over this file: 0.61 (C = 256), 0.59 on the fixture scenes, 0.22 at the OPV2V shape."""
import numpy as np
import pytest
import torch

from _lift_splat import MATRICES, SCENES, grid_conf, rig, scene, yaw_rot
from quantv2x_amd import lift_splat as ls

pytestmark = pytest.mark.gpu

SMALL = dict(final_dim=(32, 48), downsample=8)                     # a 4 x 6 feature map
GRID = {"xbound": [-16, 16, 1], "ybound": [-16, 16, 1], "zbound": [-3, 3, 6], "ddiscr": [2, 24, 8], "mode": "LID"}


def stage_for(gc, final_dim, downsample, features, m):
    b, n = m["rots"].shape[:2]
    return ls.GpuLiftSplat(gc, final_dim, downsample, features, n, b).plan(*(torch.tensor(m[k]).cuda() for k in MATRICES))


def statement_cells(stage, m):
    return ls.cells_statement(ls.geometry_statement(stage.frustum, *(m[k] for k in MATRICES)), stage.dx, stage.bx, stage.nx)


def inputs(stage, seed, scale=2.0):
    g = np.random.default_rng(seed)
    v = stage.samples * stage.views
    return ((g.standard_normal((v, stage.depth_bins, stage.fh, stage.fw)) * scale).astype(np.float32),
            g.standard_normal((v, stage.features, stage.fh, stage.fw)).astype(np.float32))


def splat(stage, depth, feats, mode="logits"):
    stage.out.fill_(float("nan"))                                  # every element must be written: the caller does not clear
    out = stage(torch.tensor(depth).cuda(), torch.tensor(feats).cuda(), mode).cpu().numpy()
    assert np.isfinite(out).all()
    return out


def within_bound(out, cells, depth, feats, mode, nx, extra=0.0, against=None, what=""):
    """every element within the derived bound of the statement (or of ``against``, with ``extra`` added) -> the largest ratio to the bound"""
    want, mag, count = ls.splat_terms_statement(cells, depth, feats, mode, nx=nx)
    bound = ls.splat_bound(count, mag, feats.shape[1], float(np.abs(feats).max()))
    diff = np.abs(out.astype(np.float64) - (want if against is None else against.astype(np.float64)))
    allowed = bound + extra                                        # what the assertion below allows, per element
    ratio = float((diff[allowed > 0] / allowed[allowed > 0]).max()) if (allowed > 0).any() else 0.0
    print(f"{what}: largest |out - want| {diff.max():.3g}, largest ratio to what is allowed {ratio:.3g}, largest cell {int(count.max())} points, "
          f"occupied {int((count > 0).sum())}")
    assert (diff <= allowed).all(), f"{what}: {int((diff > allowed).sum())} elements outside the bound, worst ratio {ratio:.3g}"
    assert not out[np.repeat(count, feats.shape[1], axis=1) == 0].view(np.int32).any(), f"{what}: an empty cell is not +0"
    return ratio


@pytest.mark.parametrize("name", SCENES)
def test_fixture_scene(name):
    s = scene(name)
    m = {k: s[k] for k in MATRICES}
    stage = stage_for(grid_conf(s), tuple(int(v) for v in s["final_dim"]), int(s["downsample"]), int(s["features"]), m)
    assert np.array_equal(stage.frustum.cpu().numpy(), s["frustum"])
    cells = stage.cells.cpu().numpy()
    assert np.array_equal(cells, statement_cells(stage, m)) and np.array_equal(cells, s["cells"])
    out = splat(stage, s["logits"], s["feats"])
    within_bound(out, cells, s["logits"], s["feats"], "logits", s["nx"], what=f"scene {name} against the statement")
    within_bound(out, cells, s["logits"], s["feats"], "logits", s["nx"], extra=4 * float(s["pool_gap"]), against=s["bev"],
                 what=f"scene {name} against the reference")


def test_every_point_outside_the_grid():
    gc = dict(GRID, xbound=[1000, 1008, 1])
    m = rig(1, 2, SMALL["final_dim"])
    stage = stage_for(gc, **SMALL, features=8, m=m)
    assert (stage.cells.cpu().numpy() == -1).all() and (statement_cells(stage, m) == -1).all()
    stage.out.fill_(float("nan"))
    out = stage(*(torch.from_numpy(a).cuda() for a in inputs(stage, 1))).cpu().numpy()
    assert out.shape == (1, 8, 32, 8) and not out.view(np.int32).any()          # +0 everywhere, from a buffer of NaN


def big_cell_rig():
    """cameras 0 and 1 put their whole frusta (2 x 48 x 6 x 8 points) into cell (0, 0) of a 2 x 2 x 1 grid of 100 m cells; camera 2 hangs
    85.4 m up over the neighbour cell (1, 0), rolled by 0.2 rad, so that exactly one of its points -- the lowest corner pixel at the
    farthest depth bin -- dips below the grid's top at z = 50 m"""
    m = rig(1, 3, (48, 64), spread=False)
    c, s = np.cos(0.2), np.sin(0.2)
    m["rots"][0, 1] = yaw_rot(0.4)
    m["rots"][0, 2] = (np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) @ yaw_rot(0.0).astype(np.float64)).astype(np.float32)
    m["trans"][0] = [[-60, -50, 1.5], [-70, -60, 1.5], [40, -50, 85.4]]
    return m


def test_one_cell_holds_two_whole_frusta_and_its_neighbour_one_point():
    gc = {"xbound": [-100, 100, 100], "ybound": [-100, 100, 100], "zbound": [-50, 50, 100], "ddiscr": [2, 50, 48], "mode": "LID"}
    m = big_cell_rig()
    stage = stage_for(gc, (48, 64), 8, 8, m)
    cells = stage.cells.cpu().numpy()
    assert np.array_equal(cells, statement_cells(stage, m))
    assert (cells[0, :2] == 0).all() and cells[0, :2].size == 4608 and (cells[0, 2] == 1).sum() == 1 and (cells[0, 2] == -1).sum() == 2303
    depth, feats = inputs(stage, 2)
    out = splat(stage, depth, feats)
    within_bound(out, cells, depth, feats, "logits", stage.nx, what="4 608 points in one cell")
    assert (out[0, :, 0, 0] != 0).all() and (out[0, :, 0, 1] != 0).all() and not out[0, :, 1, :].view(np.int32).any()
    d, h, w = (int(v[0]) for v in np.nonzero(cells[0, 2] == 1))    # the neighbour's one point: a single product, exact in fp32
    p = ls.depth_probs_statement(depth)[2, d, h, w].astype(np.float32)
    assert np.array_equal(out[0, :, 0, 1], p * feats[2, :, h, w])


def test_two_height_cells_interleave_channels():
    gc = dict(GRID, zbound=[-4, 4, 4])
    m = rig(1, 2, SMALL["final_dim"], seed=3)
    stage = stage_for(gc, **SMALL, features=8, m=m)
    cells = stage.cells.cpu().numpy()
    assert np.array_equal(cells, statement_cells(stage, m))
    depth, feats = inputs(stage, 3)
    out = splat(stage, depth, feats)
    assert out.shape == (1, 16, 32, 32)
    within_bound(out, cells, depth, feats, "logits", stage.nx, what="Z = 2")
    count = ls.splat_terms_statement(cells, depth, feats, nx=stage.nx)[2][0]                  # [Z, Y, X]
    upper_only, lower_only = (count[1] > 0) & (count[0] == 0), (count[0] > 0) & (count[1] == 0)
    assert upper_only.any() and lower_only.any()
    assert not out[0, :8][:, upper_only].any() and (out[0, 8:][:, upper_only] != 0).all()       # channel z * C + c
    assert not out[0, 8:][:, lower_only].any() and (out[0, :8][:, lower_only] != 0).all()


@pytest.mark.parametrize("features", [8, 64, 128, 256])
def test_feature_counts_served(features):
    m = rig(1, 2, SMALL["final_dim"], seed=4)
    # 70 cells a row: whole tiles of TX = min(64, 4096 / C) cells (64 / 64 / 32 / 16) and a partial one at every C
    stage = stage_for(dict(GRID, xbound=[-35, 35, 1]), **SMALL, features=features, m=m)
    cells = stage.cells.cpu().numpy()
    assert np.array_equal(cells, statement_cells(stage, m)) and (cells >= 0).any()
    depth, feats = inputs(stage, features)
    within_bound(splat(stage, depth, feats), cells, depth, feats, "logits", stage.nx, what=f"C = {features}")


def test_feature_count_refused():
    from quantv2x_amd.lib import Qv2xError
    with pytest.raises(Qv2xError, match="features 12"):
        ls.GpuLiftSplat(GRID, **SMALL, features=12, views=2)
    with pytest.raises(Qv2xError, match="features 264"):
        ls.GpuLiftSplat(GRID, **SMALL, features=264, views=2)
    with pytest.raises(Qv2xError, match="plan"):
        ls.GpuLiftSplat(GRID, **SMALL, features=8, views=2)(torch.zeros(2, 8, 4, 6), torch.zeros(2, 8, 4, 6))


def test_two_samples_with_different_cameras():
    m = rig(2, 3, SMALL["final_dim"], seed=5)
    stage = stage_for(GRID, **SMALL, features=8, m=m)
    cells = stage.cells.cpu().numpy()
    assert np.array_equal(cells, statement_cells(stage, m)) and not np.array_equal(cells[0], cells[1])
    depth, feats = inputs(stage, 5)
    out = splat(stage, depth, feats)
    for s in range(2):                                             # per sample, against the statement of that sample alone
        one = {k: v[s:s + 1] for k, v in m.items()}
        alone = ls.cells_statement(ls.geometry_statement(stage.frustum, *(one[k] for k in MATRICES)), stage.dx, stage.bx, stage.nx)
        assert np.array_equal(alone, cells[s:s + 1])
        within_bound(out[s:s + 1], alone, depth[3 * s:3 * s + 3], feats[3 * s:3 * s + 3], "logits", stage.nx, what=f"sample {s}")


def test_extreme_logits_and_one_hot_probabilities():
    m = rig(1, 2, SMALL["final_dim"], seed=6)
    stage = stage_for(GRID, **SMALL, features=8, m=m)
    cells = stage.cells.cpu().numpy()
    g = np.random.default_rng(6)
    depth, feats = inputs(stage, 6)
    depth = np.where(g.random(depth.shape) < 0.5, np.float32(80), np.float32(-80)) + depth        # spread 160 and more
    within_bound(splat(stage, depth, feats), cells, depth, feats, "logits", stage.nx, what="logits of +-80")
    hot = np.zeros_like(depth)
    np.put_along_axis(hot, g.integers(0, stage.depth_bins, (2, 1, stage.fh, stage.fw)), 1.0, axis=1)
    whole = np.rint(feats * 8).astype(np.float32)                  # small integers: every term is 1 * f or 0 * f and every partial sum is exact
    out = splat(stage, hot, whole, "probs")
    assert np.array_equal(out.astype(np.float64), ls.splat_statement(cells, hot, whole, "probs", nx=stage.nx)) and out.any()


def test_a_nan_translation_drops_that_view_alone():
    m = rig(1, 3, SMALL["final_dim"], seed=7)
    clean = stage_for(GRID, **SMALL, features=8, m=m).cells.cpu().numpy()
    bad = {k: v.copy() for k, v in m.items()}
    bad["trans"][0, 1, 2] = np.nan
    stage = stage_for(GRID, **SMALL, features=8, m=bad)
    cells = stage.cells.cpu().numpy()
    assert (clean[0, 1] >= 0).any() and (cells[0, 1] == -1).all() and np.array_equal(cells[0, [0, 2]], clean[0, [0, 2]])
    assert np.array_equal(cells, statement_cells(stage, bad))
    depth, feats = inputs(stage, 7)
    within_bound(splat(stage, depth, feats), cells, depth, feats, "logits", stage.nx, what="one view dropped")


def test_calls_repeat_bit_for_bit_eager_and_replayed():
    from quantv2x_amd.engine import capture_call
    s = scene("a")
    m = {k: s[k] for k in MATRICES}
    stage = stage_for(grid_conf(s), tuple(int(v) for v in s["final_dim"]), int(s["downsample"]), int(s["features"]), m)
    depth, feats = torch.tensor(s["logits"]).cuda(), torch.tensor(s["feats"]).cuda()
    first = stage(depth, feats).clone()
    stage.out.fill_(float("nan"))
    assert torch.equal(stage(depth, feats), first)                 # two eager calls
    replay = capture_call(lambda: stage(depth, feats))
    d2, f2 = inputs(stage, 8)
    depth.copy_(torch.from_numpy(d2))                               # the inputs refreshed in place
    feats.copy_(torch.from_numpy(f2))
    stage.out.fill_(float("nan"))
    replayed = replay().clone()
    stage.out.fill_(float("nan"))
    eager = stage(depth, feats)
    assert torch.equal(replayed, eager) and not torch.equal(eager, first)


def test_opv2v_shape_against_the_statement():
    """1 sample, 4 cameras, 48 depth bins, a 48 x 64 feature map, 64 features, the OPV2V grid: 589 824 points"""
    gc = {"xbound": [-51.2, 51.2, 0.4], "ybound": [-51.2, 51.2, 0.4], "zbound": [-10, 10, 20], "ddiscr": [2, 50, 48], "mode": "LID"}
    m = rig(1, 4, (384, 512), seed=9)
    stage = stage_for(gc, (384, 512), 8, 64, m)
    cells = stage.cells.cpu().numpy()
    assert cells.size == 589824 and np.array_equal(cells, statement_cells(stage, m))
    depth, feats = inputs(stage, 9)
    within_bound(splat(stage, depth, feats), cells, depth, feats, "logits", stage.nx, what="OPV2V shape")
