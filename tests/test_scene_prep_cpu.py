"""Scene preparation on the host: the numpy statements (``plugin.utils.pcd_utils``, ``plugin.utils.transformation_utils``, the fixed-order
solve) against ``tests/golden/scene_prep.npz`` -- the reference's own functions, recorded by ``tests/golden/make_golden_scene.py`` -- and the
shim lookup of ``opencood.utils.pcd_utils``."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _scene_common import bits, statement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# to_ego = solve4(T_0, T_a) against the reference's x1_to_x2 (inv, then dot), pairwise = solve4(T_j, T_i) against its np.linalg.solve: the
# largest absolute difference over the fixture, measured where the fixture was made: 2.07e-13 m and 1.43e-13 m (translations up to
# 1000 m relative to the world, ~120 m between agents; 1000 m * 2^-52 = 2.2e-13).  Allowed: four times that, for another LAPACK build.
TO_EGO_MEASURED, PAIRWISE_MEASURED = 2.07e-13, 1.43e-13
TO_EGO_ALLOWED, PAIRWISE_ALLOWED = 4 * TO_EGO_MEASURED, 4 * PAIRWISE_MEASURED
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def fx(golden):
    return golden["scene_prep"]


def test_the_allowance_stays_below_a_nanometre():
    assert TO_EGO_ALLOWED < 1e-9 and PAIRWISE_ALLOWED < 1e-9


def test_mask_ego_points_keeps_and_removes_exactly_the_reference_rows(fx):
    from quantv2x_amd.plugin.utils.pcd_utils import kept_rows, mask_ego_points, prepare_sweep, sentinel_row
    for k, n in enumerate(fx["sweep_points"]):
        pts, want = fx["sweeps"][k, :n], fx["ref_kept"][k, :n]
        assert 0 < want.sum() < n
        np.testing.assert_array_equal(mask_ego_points(pts), pts[want])
        out = prepare_sweep(pts, None, True)
        np.testing.assert_array_equal(bits(out[want]), bits(pts[want]))                   # kept: untouched, in place
        assert (bits(out[~want]) == bits(sentinel_row())).all()                           # removed: the sentinel's bit pattern
        np.testing.assert_array_equal(kept_rows(out), pts[want])
        np.testing.assert_array_equal(bits(prepare_sweep(pts, None, False)), bits(pts))   # no mask, no transform: a copy


def test_the_boundary_points_of_the_ego_box(fx):
    """on each float32 bound and one step inside: removed; one step outside: kept (the fixture holds all twelve in every sweep)"""
    from quantv2x_amd.plugin.utils.pcd_utils import EGO_BOX
    pts, kept = fx["sweeps"][0, :fx["sweep_points"][0]], fx["ref_kept"][0, :fx["sweep_points"][0]]
    for axis, b, out in ((0, EGO_BOX[0], -1), (0, EGO_BOX[1], 1), (1, EGO_BOX[2], -1), (1, EGO_BOX[3], 1)):
        b32 = np.float32(b)
        for v, want in ((b32, False), (np.nextafter(b32, np.float32(-out * np.inf)), False), (np.nextafter(b32, np.float32(out * np.inf)), True)):
            rows = np.nonzero(pts[:, axis] == v)[0]
            assert len(rows) == 1 and bool(kept[rows[0]]) == want, (axis, b, v)


def test_nan_rows_and_mask_points_by_range_and_shuffle(fx):
    from quantv2x_amd.plugin.utils.pcd_utils import mask_points_by_range, prepare_sweep, sentinel_row, shuffle_points
    pts = fx["sweeps"][1, :200].copy()
    pts[5, 0], pts[9, 2], pts[11] = np.nan, np.nan, sentinel_row()
    out = prepare_sweep(pts, fx["sweep_transforms"][1], False)
    assert (bits(out[[5, 9, 11]]) == bits(sentinel_row())).all() and not np.isnan(np.delete(out, [5, 9, 11], 0)).any()
    rng = [-20.0, -10.0, -2.0, 30.0, 15.0, 0.5]
    m = mask_points_by_range(pts, rng)
    ok = (pts[:, 0] > -20) & (pts[:, 0] < 30) & (pts[:, 1] > -10) & (pts[:, 1] < 15) & (pts[:, 2] > -2) & (pts[:, 2] < 0.5)
    np.testing.assert_array_equal(m, pts[ok])
    np.random.seed(3)
    s = shuffle_points(fx["sweeps"][2, :300])
    assert sorted(s[:, 3].tolist()) == sorted(fx["sweeps"][2, :300, 3].tolist()) and not np.array_equal(s, fx["sweeps"][2, :300])


def test_projected_points_within_the_fp32_chain_bound(fx):
    """|x' - reference| <= 16 * 2^-24 * M per coordinate, M = |m00 x| + |m01 y| + |m02 z| + |m03|: the reference evaluates three products
    and three sums in fp32 on a matrix rounded to fp32 (about 8 u M), doubled.  Measured on the fixture: at most 2.57 u M."""
    from quantv2x_amd.plugin.utils.pcd_utils import kept_rows, prepare_sweep
    worst = 0.0
    for k, n in enumerate(fx["sweep_points"]):
        pts, tf = fx["sweeps"][k, :n], fx["sweep_transforms"][k]
        kept = fx["ref_kept"][k, :n]
        got = kept_rows(prepare_sweep(pts, tf, True))
        assert got.shape[0] == kept.sum()
        np.testing.assert_array_equal(got[:, 3], pts[kept][:, 3])                            # order and intensity untouched
        m = tf.astype(np.float32).astype(np.float64)
        M = np.abs(pts[kept][:, :3].astype(np.float64)) @ np.abs(m[:3, :3]).T + np.abs(m[:3, 3])
        d = np.abs(got[:, :3].astype(np.float64) - fx["ref_projected"][k, :kept.sum()].astype(np.float64))
        worst = max(worst, float((d / (U24 * M)).max()))
        assert (d <= 16 * U24 * M).all(), (k, worst)
    print("projection: worst", worst, "u M")


def test_select_in_range_is_exact(fx):
    from quantv2x_amd.plugin.utils.pcd_utils import select_in_range
    comm = float(fx["comm_range"])
    for k, n in enumerate(fx["range_counts"]):
        want = np.nonzero(fx["ref_in_range"][k, :n])[0].tolist()
        assert select_in_range(fx["range_poses"][k, :n], comm) == want, k
        assert 0 in want and len(want) < n
    assert fx["ref_in_range"][fx["range_deliberate"]].sum() == 7 and (~fx["ref_in_range"][fx["range_deliberate"]]).sum() == 6


def test_x_to_world_is_exact_and_x1_to_x2_is_the_references(fx):
    from quantv2x_amd.plugin.utils.transformation_utils import get_pairwise_transformation, x1_to_x2, x_to_world
    for s, n in enumerate(fx["counts"]):
        for a in range(n):
            np.testing.assert_array_equal(x_to_world(fx["poses"][s, a]), fx["ref_world"][s, a])
            assert np.abs(x1_to_x2(fx["poses"][s, a], fx["poses"][s, 0]) - fx["ref_to_ego"][s, a]).max() <= TO_EGO_ALLOWED
        base = {a: {"params": {"lidar_pose": fx["poses"][s, a]}} for a in range(n)}
        assert np.abs(get_pairwise_transformation(base, 5, False) - fx["ref_pairwise"][s]).max() <= PAIRWISE_ALLOWED
        np.testing.assert_array_equal(get_pairwise_transformation(base, 5, True), fx["ref_pairwise_proj"][s])


def test_the_fixed_order_solve_against_the_references_inverse_and_solve(fx):
    st = statement(fx["poses"], fx["counts"])
    np.testing.assert_array_equal(st["world"], fx["ref_world"])
    d_ego, d_pair = float(np.abs(st["to_ego"] - fx["ref_to_ego"]).max()), float(np.abs(st["pairwise"] - fx["ref_pairwise"]).max())
    print("to_ego: largest difference", d_ego, "m; pairwise:", d_pair, "m")
    assert d_ego <= TO_EGO_ALLOWED and d_pair <= PAIRWISE_ALLOWED
    assert np.abs(fx["poses"][..., :2]).max() == 1000.0                                    # at the fixture's 1000 m magnitudes
    proj = statement(fx["poses"], fx["counts"], proj_first=True)
    np.testing.assert_array_equal(proj["pairwise"], fx["ref_pairwise_proj"])
    np.testing.assert_array_equal(proj["to_ego"], st["to_ego"])
    for s in range(len(fx["counts"])):                                                    # to_ego[a] is pairwise[a][0]
        np.testing.assert_array_equal(st["to_ego"][s, 1:], st["pairwise"][s, 1:, 0])


SHIM = r'''
import sys
assert not any("reference" in p for p in sys.path), sys.path
import opencood, os
assert os.path.dirname(opencood.__file__).endswith(os.path.join("integration", "opencood")), opencood.__file__
from opencood.utils.pcd_utils import mask_ego_points, mask_points_by_range, shuffle_points
from opencood.utils.transformation_utils import x1_to_x2, x_to_world, get_pairwise_transformation
import quantv2x_amd.plugin.utils.pcd_utils as p, quantv2x_amd.plugin.utils.transformation_utils as t
assert mask_ego_points is p.mask_ego_points and mask_points_by_range is p.mask_points_by_range and shuffle_points is p.shuffle_points
assert x1_to_x2 is t.x1_to_x2
print("shim ok")
'''


def test_the_shim_resolves_the_reference_names_of_this_stage():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "integration"), ROOT])
    r = subprocess.run([sys.executable, "-c", SHIM], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "shim ok" in r.stdout, r.stderr[-3000:]
