"""The lift-splat statements (quantv2x_amd/lift_splat.py) and the reference-named camera helpers against tests/golden/lift_splat.npz --
the reference's own ``create_frustum``, ``get_geometry`` and ``voxel_pooling`` on three tiny scenes -- and the host-side limits of the C
entries.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from _lift_splat import MATRICES, SCENES, grid_conf, scene
from quantv2x_amd import lift_splat as ls
from quantv2x_amd.plugin.utils.camera_utils import depth_discretization, gen_dx_bx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", SCENES)
def test_grid_bins_and_frustum_are_bit_equal(name):
    s = scene(name)
    gc = grid_conf(s)
    dx, bx, nx = gen_dx_bx(gc["xbound"], gc["ybound"], gc["zbound"])
    assert dx.numpy().dtype == np.float32 and bx.numpy().dtype == np.float32 and nx.numpy().dtype == np.int64
    assert np.array_equal(dx.numpy(), s["dx"]) and np.array_equal(bx.numpy(), s["bx"]) and np.array_equal(nx.numpy(), s["nx"])
    bins = depth_discretization(*gc["ddiscr"], gc["mode"])
    assert bins.dtype == np.float64 and np.array_equal(bins, s["depth_bins"])
    fr = ls.create_frustum(tuple(s["final_dim"]), int(s["downsample"]), gc["ddiscr"], gc["mode"]).numpy()
    assert fr.dtype == np.float32 and fr.shape == s["frustum"].shape and np.array_equal(fr, s["frustum"])


def test_depth_discretization_modes():
    ud, lid = depth_discretization(2, 50, 48, "UD"), depth_discretization(2, 50, 48, "LID")
    assert ud[0] == lid[0] == 2 and np.all(np.diff(ud) == np.diff(ud)[0]) and np.all(np.diff(lid, 2) > 0)
    with pytest.raises(NotImplementedError):
        depth_discretization(2, 50, 48, "SID")


@pytest.mark.parametrize("name", SCENES)
def test_cells_equal_the_references_on_every_point(name):
    s = scene(name)
    geom = ls.geometry_statement(s["frustum"], *(s[k] for k in MATRICES))
    assert geom.dtype == np.float32 and geom.shape == s["geom"].shape
    gap = float(np.sqrt(((geom.astype(np.float64) - s["geom"]) ** 2).sum(-1)).max())
    assert gap <= float(s["geom_gap"]) + 2.0 ** -23 * 64          # the statement is the rounded float64 chain: the stored gap plus one rounding
    cells = ls.cells_statement(geom, s["dx"], s["bx"], s["nx"])
    assert cells.dtype == np.int32 and np.array_equal(cells, s["cells"])
    # the fixture has what it promises: points kept only through the truncation, points dropped on both sides
    assert int(s["kept_by_truncation"]) > 0 and int(s["dropped_below"]) > 0 and int(s["dropped_above"]) > 0
    assert float(s["margin"]) > 8 * float(s["geom_gap"])


@pytest.mark.parametrize("name", SCENES)
def test_splat_statement_against_the_references_pooling(name):
    s = scene(name)
    want, _, count = ls.splat_terms_statement(s["cells"], s["logits"], s["feats"], "logits", nx=s["nx"])
    assert want.dtype == np.float64 and want.shape == s["bev"].shape
    gap = float(np.abs(want - s["bev"]).max())
    print(f"scene {name}: statement to reference {gap:.3g}, stored pool_gap {float(s['pool_gap']):.3g}")
    assert gap <= 4 * float(s["pool_gap"])                         # four: another torch build's softmax and cumsum (DESIGN.md section 11's factor)
    b, (x, y, z) = want.shape[0], (int(v) for v in s["nx"])
    assert np.array_equal((s["bev"].reshape(b, z, -1, y, x) != 0).any(2), count > 0)      # the same cells are occupied


def test_truncation_toward_zero_keeps_half_a_cell_below_the_range():
    dx, bx, nx = gen_dx_bx([-4, 4, 1], [-4, 4, 1], [-2, 2, 4])
    lo = np.array([-4.0, -4.0, -2.0], np.float32)
    mid = lo + np.float32(0.5) * dx.numpy()
    pts = np.stack([mid + np.array([-1.0, 0, 0], np.float32),      # -0.5 cell on x: kept, cell 0
                    mid + np.array([-1.5, 0, 0], np.float32),      # -1.0 cell: dropped
                    mid + np.array([7.5, 0, 0], np.float32),       # exactly nx: dropped
                    mid + np.array([7.0, 0, 0], np.float32),       # the last cell
                    mid + np.array([0, 0, -4.0], np.float32),      # -0.5 cell on z (a 4 m cell): kept
                    mid + np.array([0, -1.0, -4.0], np.float32),   # -0.5 cell on y and z: kept
                    np.array([np.nan, 0, 0], np.float32), np.array([0, np.inf, 0], np.float32), np.array([0, 0, -np.inf], np.float32)])
    cells = ls.cells_statement(pts.reshape(1, 1, 9, 1, 1, 3), dx, bx, nx).reshape(-1)
    assert cells.tolist() == [0, -1, -1, 7, 0, 0, -1, -1, -1]


def test_splat_statement_layout_and_modes():
    """two points in cell (x 1, y 2, z 1) of a 3 x 4 x 2 grid: channel z * C + c, map [Y, X]; one-hot probabilities pass through"""
    nx = np.array([3, 4, 2])
    cells = np.full((1, 1, 2, 1, 2), -1, np.int32)
    cells[0, 0, 1, 0, 0] = cells[0, 0, 0, 0, 1] = (1 * 4 + 2) * 3 + 1
    probs = np.zeros((1, 2, 1, 2), np.float32)
    probs[0, 1, 0, 0] = probs[0, 0, 0, 1] = 1.0
    feats = np.arange(1, 17, dtype=np.float32).reshape(1, 8, 1, 2)
    out, mag, count = ls.splat_terms_statement(cells, probs, feats, "probs", nx=nx)
    assert out.shape == (1, 16, 4, 3) and count.shape == (1, 2, 4, 3) and count[0, 1, 2, 1] == 2 and count.sum() == 2
    assert np.array_equal(out[0, 8:, 2, 1], feats[0, :, 0, 0] + feats[0, :, 0, 1]) and np.count_nonzero(out) == 8
    assert np.array_equal(mag, np.abs(out))
    soft = ls.splat_statement(cells, np.zeros_like(probs), feats, "logits", nx=nx)      # equal logits: probability 1/2 each
    assert np.allclose(soft, out / 2, rtol=1e-15)


SHIM = r'''
import sys
assert not any("reference" in p for p in sys.path), sys.path
import opencood, os
assert os.path.dirname(opencood.__file__).endswith(os.path.join("integration", "opencood")), opencood.__file__
from opencood.utils.camera_utils import gen_dx_bx, depth_discretization
import quantv2x_amd.plugin.utils.camera_utils as m
assert gen_dx_bx is m.gen_dx_bx and depth_discretization is m.depth_discretization
print("shim ok")
'''


def test_shim_resolves_camera_utils():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "integration"), ROOT])
    r = subprocess.run([sys.executable, "-c", SHIM], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "shim ok" in r.stdout, r.stderr[-3000:]


def _desc(**kw):
    from quantv2x_amd import lib
    d = lib.LssDesc()
    v = dict(samples=1, views=4, depth_bins=48, fh=48, fw=64, features=128, nx=(256, 256, 1), dx=(0.4, 0.4, 20.0), bx=(-51.0, -51.0, 0.0))
    v.update(kw)
    d.samples, d.views, d.depth_bins, d.fh, d.fw, d.features = v["samples"], v["views"], v["depth_bins"], v["fh"], v["fw"], v["features"]
    for i in range(3):
        d.nx[i], d.dx[i], d.bx[i] = v["nx"][i], v["dx"][i], v["bx"][i]
    return d


def test_c_entries_refuse_what_is_outside_the_limits():
    """checked on the host before any GPU call, with an error that names the offending value"""
    from quantv2x_amd import lib
    l = lib.load()
    err = lambda: l.qv2x_last_error().decode()                      # noqa: E731
    assert l.qv2x_lss_workspace_bytes(C.byref(_desc())) > 0
    for kw, word in ((dict(features=12), "features 12"), (dict(features=264), "features 264"), (dict(features=0), "features 0"),
                     (dict(samples=13, views=5), "samples 13 x views 5"), (dict(depth_bins=129), "depth_bins 129"),
                     (dict(nx=(65536, 32768, 1)), "cells exceed int32"), (dict(samples=16, fh=1024, fw=1024), "frustum points exceed int32"),
                     (dict(nx=(256, 0, 1)), "nx[1] = 0"), (dict(dx=(0.4, -0.4, 20.0)), "dx[1] = -0.4"), (dict(fh=0), "feature map 0 x 64")):
        d = _desc(**kw)
        assert l.qv2x_lss_workspace_bytes(C.byref(d)) == -1 and word in err(), (kw, err())
        one = C.c_void_p(16)                                        # never dereferenced: the descriptor is refused first
        assert l.qv2x_lss_plan_f32(C.byref(d), one, one, one, one, one, one, one, one, None) == -1 and word in err()
        assert l.qv2x_lss_splat_f32(C.byref(d), one, one, 0, one, one, None) == -1 and word in err()
    d, one = _desc(), C.c_void_p(16)
    assert l.qv2x_lss_workspace_bytes(None) == -1
    assert l.qv2x_lss_plan_f32(C.byref(d), one, one, one, None, one, one, one, one, None) == -1 and "null pointer" in err()
    assert l.qv2x_lss_splat_f32(C.byref(d), one, one, 2, one, one, None) == -1 and "mode 2" in err()
    assert l.qv2x_lss_splat_f32(C.byref(d), one, one, 0, C.c_void_p(8), one, None) == -2 and "16-byte" in err()
    assert l.qv2x_lss_splat_f32(C.byref(d), None, one, 0, one, one, None) == -1 and "null pointer" in err()
