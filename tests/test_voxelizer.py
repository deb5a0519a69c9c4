"""Pillar voxelizer contract: numpy generator (synth) and GPU kernel against the plain-Python statement in oracle/."""
import numpy as np
import pytest

from oracle.voxelize import voxelize as ref_voxelize
from quantv2x_amd import synth

RANGE, VS = synth.SHAPES["tiny"][0], synth.SHAPES["tiny"][1]


def _cloud(n, seed, sigma=6.0):
    g = np.random.default_rng(seed)
    pts = np.stack([g.normal(0, sigma, n), g.normal(0, sigma / 2, n), g.uniform(-3.5, 1.5, n), g.uniform(0, 1, n)], 1)
    return pts.astype(np.float32)     # includes out-of-range points on purpose


@pytest.mark.parametrize("n,max_points,max_voxels", [(500, 32, 2048), (5000, 32, 2048), (5000, 4, 100), (0, 32, 16)])
def test_numpy_voxelizer_follows_contract(n, max_points, max_voxels):
    pts = _cloud(max(n, 1), 1)[:n]
    f, c, m = synth.voxelize(pts, RANGE, VS, max_points, max_voxels) if n else ref_voxelize(pts, RANGE, VS, max_points, max_voxels)
    rf, rc, rm = ref_voxelize(pts, RANGE, VS, max_points, max_voxels)
    np.testing.assert_array_equal(f, rf); np.testing.assert_array_equal(c, rc); np.testing.assert_array_equal(m, rm)


@pytest.mark.gpu
@pytest.mark.parametrize("n,max_points,max_voxels", [(1, 32, 64), (700, 32, 2048), (6000, 32, 2048), (6000, 4, 100)])
def test_gpu_voxelizer_small(n, max_points, max_voxels):
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    pts = _cloud(n, 2)
    rf, rc, rm = ref_voxelize(pts, RANGE, VS, max_points, max_voxels)
    f, c, m = GpuVoxelizer(RANGE, VS, max_points, max_voxels).one(torch.from_numpy(pts).cuda(), agent=3)
    np.testing.assert_array_equal(m.cpu().numpy(), rm)
    np.testing.assert_array_equal(c.cpu().numpy()[:, 1:], rc)
    assert (c.cpu().numpy()[:, 0] == 3).all()
    np.testing.assert_array_equal(f.cpu().numpy(), rf)


def _edge_sweep(case):
    """the smallest sweeps of the one-sweep key layout -> (points, max_points, max_voxels)"""
    g = np.random.default_rng(7)
    lo, hi, vs = np.asarray(RANGE[:3]), np.asarray(RANGE[3:]), np.asarray(VS)
    if case == "one_point":
        return np.array([[lo[0] + 2.5 * vs[0], hi[1] - 0.5 * vs[1], -1.0, 0.5]], np.float32), 32, 64
    if case == "all_outside":
        pts = _cloud(300, 3)
        pts[:150, 0] = hi[0] + g.uniform(0.01, 5.0, 150)                 # beyond +x
        pts[150:, 1] = lo[1] - g.uniform(0.01, 5.0, 150)                 # beyond -y
        return pts, 32, 64
    cells = g.choice(int((hi[0] - lo[0]) / vs[0]) * int((hi[1] - lo[1]) / vs[1]), size=40, replace=False)       # "both_caps"
    nx = int((hi[0] - lo[0]) / vs[0])
    centre = np.stack([lo[0] + (cells % nx + 0.5) * vs[0], lo[1] + (cells // nx + 0.5) * vs[1]], 1)
    of = g.integers(0, 40, 2000)
    xy = centre[of] + g.uniform(-0.3, 0.3, (2000, 2)) * vs[:2]
    return np.concatenate([xy, g.uniform(-2.5, 0.5, (2000, 1)), g.uniform(0, 1, (2000, 1))], 1).astype(np.float32), 4, 16


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one_point", "all_outside", "both_caps"])
def test_gpu_voxelizer_one_sweep_edge_shapes(case):
    """``one`` and ``fixed([pts], cap)`` -- a batch of ONE sweep underneath -- against the plain-Python contract, exactly: a single valid
    point; no valid point at all (count 0, every row in the defined tail state); ~40 cells of 50 points with 16 voxels of 4 points allowed
    (the voxel cap and the per-voxel cap both bite)."""
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    pts, max_points, max_voxels = _edge_sweep(case)
    rf, rc, rm = ref_voxelize(pts, RANGE, VS, max_points, max_voxels)
    full = ref_voxelize(pts, RANGE, VS, 10 ** 6, 10 ** 6)[2]            # on the CPU: the sweep is the case it is meant to be
    assert {"one_point": len(pts) == 1 and len(rm) == 1, "all_outside": len(pts) == 300 and len(rm) == 0,
            "both_caps": len(pts) == 2000 and 35 <= len(full) <= 40 and len(rm) == 16 and full[:16].min() > 4}[case]
    vz = GpuVoxelizer(RANGE, VS, max_points, max_voxels)
    dev = torch.from_numpy(pts).cuda()
    f, c, m = vz.one(dev, agent=2)
    assert torch.equal(f.cpu(), torch.from_numpy(rf)) and torch.equal(m.cpu(), torch.from_numpy(rm))
    assert torch.equal(c.cpu()[:, 1:], torch.from_numpy(rc)) and (c[:, 0] == 2).all()
    for cap in (max_voxels, 64):
        wf, wc, wm = ref_voxelize(pts, RANGE, VS, max_points, cap)
        k = len(wm)
        o = vz.fixed([dev], cap)
        assert o["voxel_features"].shape == (cap, max_points, 4) and int(o["voxel_counts"][0]) == k
        assert torch.equal(o["voxel_features"][:k].cpu(), torch.from_numpy(wf)) and torch.equal(o["voxel_num_points"][:k].cpu(), torch.from_numpy(wm))
        assert torch.equal(o["voxel_coords"][:k, 1:].cpu(), torch.from_numpy(wc)) and (o["voxel_coords"][:k, 0] == 0).all()
        # the rows past the count: coords -1, zero points, zero features
        assert (o["voxel_coords"][k:] == -1).all() and (o["voxel_num_points"][k:] == 0).all() and (o["voxel_features"][k:] == 0).all()


@pytest.mark.gpu
def test_gpu_voxelizer_empty_sweep():
    """a sweep with no point gives no pillar (and an agent without pillars is a valid model input)"""
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    vox = GpuVoxelizer(RANGE, VS, 32, 64)
    f, c, m = vox.one(torch.empty((0, 4), dtype=torch.float32, device="cuda"), agent=0)
    assert f.shape == (0, 32, 4) and c.shape == (0, 4) and m.shape == (0,)
    both = vox([torch.empty((0, 4), dtype=torch.float32, device="cuda"), torch.from_numpy(_cloud(300, 4)).cuda()])
    assert (both["voxel_coords"][:, 0] == 1).all() and both["voxel_features"].shape[0] > 0


@pytest.mark.gpu
def test_gpu_voxelizer_full_size_feeds_the_model_inputs():
    """60k-point V2X-Real sweeps, two agents: identical to the numpy generator the rest of the suite uses."""
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    rng, vs, max_vox, _ = synth.SHAPES["v2xreal"]
    sweeps = [synth.make_points(rng, 60000, 3000 + a, 35.0) for a in range(2)]
    got = GpuVoxelizer(rng, vs, 32, max_vox)([torch.from_numpy(s).cuda() for s in sweeps])
    want = synth.make_scene("v2xreal", n_agents=2, seed=3, n_points=60000)["inputs_m1"]
    for k in ("voxel_features", "voxel_coords", "voxel_num_points"):
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg=k)


@pytest.mark.gpu
def test_fixed_capacity_form_inside_a_hip_graph_equals_the_eager_chain():
    """``GpuVoxelizer.fixed``: every sweep hands ``capacity`` rows on (tail rows: batch index -1, dropped by the PFN kernel), nothing is
    read back, so voxelizer + model replay as ONE HIP graph -- with the same predictions as the eager chain with its host-side pillar
    count, also after the sweeps' contents changed in place between replays (the clears are kernels, not memset nodes)."""
    import torch
    from _common import calibrated_plugin
    from quantv2x_amd.engine import deploy
    from quantv2x_amd.ptq_state import export_ptq_state
    from quantv2x_amd.voxelizer import GpuVoxelizer
    rng, vs, _, _ = synth.SHAPES["tiny"]
    eng = deploy(state=export_ptq_state(calibrated_plugin()))
    vz = GpuVoxelizer(rng, vs, 32, 2048)
    clouds = [[synth.make_points(rng, 3000, 50 + 2 * k + a, 6.0)[:2400].copy() for a in range(2)] for k in range(2)]   # (a graph fixes the point count)
    assert all(c.shape[0] == 2400 for cs in clouds for c in cs)
    sweeps = [torch.from_numpy(c).cuda() for c in clouds[0]]
    pairwise = torch.eye(4, dtype=torch.float64).reshape(1, 1, 1, 4, 4).repeat(1, 5, 5, 1, 1).cuda()

    def model(inp):
        return eng({"inputs_m1": inp, "agent_modality_list": ["m1", "m1"], "record_len": torch.tensor([2]), "pairwise_t_matrix": pairwise})
    fixed = vz.fixed(sweeps, 1024)
    counts = fixed["voxel_counts"].cpu().numpy()
    eager = vz(sweeps)
    m0 = int(counts[0])
    assert counts.sum() == eager["voxel_features"].shape[0] and (fixed["voxel_coords"][m0:1024, 0] == -1).all()
    assert torch.equal(fixed["voxel_features"][:m0], eager["voxel_features"][:m0]) and (fixed["voxel_num_points"][m0:1024] == 0).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model(vz.fixed(sweeps, 1024))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model(vz.fixed(sweeps, 1024))
    for k in (0, 1, 0):
        for s, c in zip(sweeps, clouds[k]):
            s.copy_(torch.from_numpy(c))
        graph.replay()
        torch.cuda.synchronize()
        want = model(vz([torch.from_numpy(c).cuda() for c in clouds[k]]))
        assert torch.equal(out["preds_tensor"], want["preds_tensor"]), k


# ---- the 70 000-voxel budget and the 32-point cap at V2X-Real size (VERDICT r4 "missing 4"; sp_voxel_preprocessor.py:38-40, 54-85) -----------
def _dense_v2xreal_cloud(n=400000, seed=11):
    """a sweep that overflows BOTH limits of the V2X-Real yaml: ~130 000 occupied cells of the 704 x 200 grid (budget 70 000) and a
    cluster of 30 000 points on ~120 cells (cap 32 points per voxel); 3 % of the points lie outside the range"""
    rng, _, _, _ = synth.SHAPES["v2xreal"]
    g = np.random.default_rng(seed)
    lo, hi = np.asarray(rng[:3]), np.asarray(rng[3:])
    pts = g.uniform(lo - 0.015 * (hi - lo), hi + 0.015 * (hi - lo), size=(n, 3))
    pts[:30000, :2] = g.normal([20.0, -5.0], [2.0, 1.0], size=(30000, 2))
    g.shuffle(pts)
    return np.concatenate([pts, g.uniform(0, 1, (n, 1))], 1).astype(np.float32)


def test_numpy_voxelizer_at_the_voxel_budget_follows_the_contract():
    """the vectorised generator the suite uses (synth.voxelize) against the plain-Python contract on the overflowing full-size sweep"""
    rng, vs, max_vox, _ = synth.SHAPES["v2xreal"]
    assert max_vox == 70000
    pts = _dense_v2xreal_cloud()
    f, c, m = synth.voxelize(pts, rng, vs, 32, max_vox)
    rf, rc, rm = ref_voxelize(pts, rng, vs, 32, max_vox)
    assert rf.shape[0] == 70000 and rm.max() == 32 and (rm == 32).sum() > 50      # both limits bite
    np.testing.assert_array_equal(c, rc); np.testing.assert_array_equal(m, rm); np.testing.assert_array_equal(f, rf)


@pytest.mark.gpu
def test_gpu_voxelizer_at_the_voxel_budget_and_point_cap_full_size():
    """qv2x_voxelize_f32 on the same sweep: exactly the first 70 000 voxels in order of first appearance, later cells dropped with all their
    points, 32 first-come points per voxel -- and the capturable fixed-capacity form hands the same rows on"""
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    rng, vs, max_vox, _ = synth.SHAPES["v2xreal"]
    pts = _dense_v2xreal_cloud()
    wf, wc, wm = synth.voxelize(pts, rng, vs, 32, max_vox)
    assert wf.shape[0] == max_vox
    vz = GpuVoxelizer(rng, vs, 32, max_vox)
    dev_pts = torch.from_numpy(pts).cuda()
    f, c, m = vz.one(dev_pts, agent=1)
    assert f.shape[0] == max_vox
    np.testing.assert_array_equal(m.cpu().numpy(), wm)
    np.testing.assert_array_equal(c.cpu().numpy()[:, 1:], wc)
    np.testing.assert_array_equal(f.cpu().numpy(), wf)
    fixed = vz.fixed([dev_pts], max_vox)
    torch.cuda.synchronize()
    assert int(fixed["voxel_counts"][0]) == max_vox
    np.testing.assert_array_equal(fixed["voxel_features"].cpu().numpy(), wf)
    # a smaller hand-on capacity than the sweep's voxels: the first `capacity` voxels, nothing written past them
    small = vz.fixed([dev_pts], 4096)
    torch.cuda.synchronize()
    assert int(small["voxel_counts"][0]) == 4096 and small["voxel_features"].shape[0] == 4096
    np.testing.assert_array_equal(small["voxel_coords"].cpu().numpy()[:, 1:], wc[:4096])
    np.testing.assert_array_equal(small["voxel_num_points"].cpu().numpy(), synth.voxelize(pts, rng, vs, 32, 4096)[2])
