"""qv2x_voxelize_batch_f32 (``GpuVoxelizer.fixed_batch``): every sweep's slab of one call equals the contract of oracle/voxelize.py and
what the per-sweep entry writes -- bit for bit, tail rows included.  Needs an MI355X."""
import numpy as np
import pytest

from oracle.voxelize import voxelize as ref_voxelize
from quantv2x_amd import synth

pytestmark = pytest.mark.gpu
RANGE, VS = synth.SHAPES["tiny"][0], synth.SHAPES["tiny"][1]
KEYS = ("voxel_features", "voxel_coords", "voxel_num_points", "voxel_counts")


def _cloud(n, seed, sigma=6.0):
    g = np.random.default_rng(seed)
    pts = np.stack([g.normal(0, sigma, n), g.normal(0, sigma / 2, n), g.uniform(-3.5, 1.5, n), g.uniform(0, 1, n)], 1)
    return pts.astype(np.float32)     # includes out-of-range points on purpose


def _dev(clouds):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() if len(c) else torch.empty((0, 4), dtype=torch.float32, device="cuda") for c in clouds]


def _check_against(out, clouds, want, max_points, capacity, first_agent=0):
    """``out``: the dict of one call; ``want[s]``: (features, coords zyx, num_points) of sweep s under the contract"""
    f, c, m, k = (out[key].cpu().numpy() for key in KEYS)
    assert f.shape == (len(clouds) * capacity, max_points, 4) and c.shape == (len(clouds) * capacity, 4) and k.shape == (len(clouds),)
    for s, (wf, wc, wm) in enumerate(want):
        n, lo = wf.shape[0], s * capacity
        assert k[s] == n, (s, k[s], n)
        np.testing.assert_array_equal(m[lo:lo + n], wm, err_msg=f"sweep {s}")
        np.testing.assert_array_equal(c[lo:lo + n, 1:], wc, err_msg=f"sweep {s}")
        assert (c[lo:lo + n, 0] == first_agent + s).all()
        np.testing.assert_array_equal(f[lo:lo + n], wf, err_msg=f"sweep {s}")
        # the defined tail: coords -1, zero points, zero features
        assert (c[lo + n:lo + capacity] == -1).all() and (m[lo + n:lo + capacity] == 0).all() and not f[lo + n:lo + capacity].any()


def test_sweeps_of_0_1_700_6000_points_in_one_call():
    """The whole-dict comparison with ``fixed`` runs on the non-empty sweeps: ``fixed`` (left as it is) refuses an empty sweep.  The call
    WITH the empty sweep, in the middle of the batch, is held against the contract oracle and, slab by slab, against ``fixed``'s rows."""
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    clouds = [_cloud(700, 2), _cloud(700, 2)[:0], _cloud(1, 5), _cloud(6000, 4)]
    want = [ref_voxelize(c, RANGE, VS, 32, 2048) for c in clouds]
    assert want[1][0].shape[0] == 0 and want[2][0].shape[0] == 1 and want[3][0].shape[0] > 1000 > want[0][0].shape[0] > 100
    vz = GpuVoxelizer(RANGE, VS, 32, 2048)
    out = vz.fixed_batch(_dev(clouds), 2048, first_agent=5)
    _check_against(out, clouds, want, 32, 2048, first_agent=5)
    full = [c for c in clouds if len(c)]
    a, b = vz.fixed_batch(_dev(full), 2048), vz.fixed(_dev(full), 2048)
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key
    for slab, s in enumerate((0, 2, 3)):                                   # the batch with the empty sweep: the same rows, its own agent column
        for key in KEYS[:3]:
            x, y = out[key][s * 2048:(s + 1) * 2048], b[key][slab * 2048:(slab + 1) * 2048]
            if key == "voxel_coords":
                x, y = x[:, 1:], y[:, 1:]
            assert torch.equal(x, y), (key, s)
        assert int(out["voxel_counts"][s]) == int(b["voxel_counts"][slab])


def test_both_caps_bite():
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    clouds = [_cloud(6000, 2), _cloud(6000, 7)]
    want = [ref_voxelize(c, RANGE, VS, 4, 100) for c in clouds]
    for wf, _, wm in want:                                                 # on the CPU first: both caps bite
        assert wf.shape[0] == 100 and (wm == 4).any()
    vz = GpuVoxelizer(RANGE, VS, 4, 100)
    out = vz.fixed_batch(_dev(clouds), 100)
    _check_against(out, clouds, want, 4, 100)
    ref = vz.fixed(_dev(clouds), 100)
    for key in KEYS:
        assert torch.equal(out[key], ref[key]), key


def test_sweeps_do_not_merge():
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    vz = GpuVoxelizer(RANGE, VS, 32, 2048)
    # the same cloud twice: identical rows in both slabs (but for the agent column)
    c = _cloud(3000, 5)
    out = vz.fixed_batch(_dev([c, c]), 1024)
    w = ref_voxelize(c, RANGE, VS, 32, 1024)
    _check_against(out, [c, c], [w, w], 32, 1024)
    for key in KEYS[:3]:
        x = out[key]
        a, b = (x[:1024, 1:], x[1024:, 1:]) if key == "voxel_coords" else (x[:1024], x[1024:])
        assert torch.equal(a, b), key
    # a sweep with every point outside the range between two ordinary ones
    far = _cloud(500, 6)
    far[:, 0] += 100.0
    clouds = [_cloud(400, 7), far, _cloud(400, 8)]
    want = [ref_voxelize(x, RANGE, VS, 32, 512) for x in clouds]
    assert want[1][0].shape[0] == 0
    _check_against(vz.fixed_batch(_dev(clouds), 512), clouds, want, 32, 512)
    # sweep s ends and sweep s + 1 begins in the same cell (and sweep s + 1 goes on in it)
    a, b = _cloud(700, 9), _cloud(700, 10)
    a[-2:] = [[0.10, 0.10, 0.0, 0.5], [0.12, 0.15, -1.0, 0.25]]
    b[:3] = [[0.15, 0.12, 0.5, 0.75], [0.11, 0.13, 0.0, 0.1], [0.2, 0.3, -2.0, 0.9]]
    want = [ref_voxelize(x, RANGE, VS, 32, 2048) for x in (a, b)]
    cell = lambda p: np.floor((p[:3] - np.asarray(RANGE[:3], np.float32)) / np.asarray(VS, np.float32))
    assert (cell(a[-1]) == cell(b[0])).all() and (cell(a[-2]) == cell(b[1])).all()
    assert want[1][2][0] >= 3
    _check_against(vz.fixed_batch(_dev([a, b]), 2048), [a, b], want, 32, 2048)


def _dense_v2xreal_cloud(n=400000, seed=11):
    """a sweep that overflows BOTH limits of the V2X-Real yaml (tests/test_voxelizer.py builds the same one): ~130 000 occupied cells of the
    704 x 200 grid (budget 70 000) and a cluster of 30 000 points on ~120 cells (cap 32 points per voxel); 3 % outside the range"""
    rng = synth.SHAPES["v2xreal"][0]
    g = np.random.default_rng(seed)
    lo, hi = np.asarray(rng[:3]), np.asarray(rng[3:])
    pts = g.uniform(lo - 0.015 * (hi - lo), hi + 0.015 * (hi - lo), size=(n, 3))
    pts[:30000, :2] = g.normal([20.0, -5.0], [2.0, 1.0], size=(30000, 2))
    g.shuffle(pts)
    return np.concatenate([pts, g.uniform(0, 1, (n, 1))], 1).astype(np.float32)


def test_full_size_three_sweeps():
    from quantv2x_amd.voxelizer import GpuVoxelizer
    rng, vs, max_vox, _ = synth.SHAPES["v2xreal"]
    assert max_vox == 70000
    clouds = [synth.make_points(rng, 60000, 3000, 35.0), _dense_v2xreal_cloud(), np.zeros((0, 4), np.float32)]
    want = [synth.voxelize(c, rng, vs, 32, max_vox) for c in clouds[:2]] + [ref_voxelize(clouds[2], rng, vs, 32, max_vox)]
    assert want[1][0].shape[0] == max_vox and (want[1][2] == 32).sum() > 50 and 10000 < want[0][0].shape[0] < max_vox
    out = GpuVoxelizer(rng, vs, 32, max_vox).fixed_batch(_dev(clouds), max_vox)
    _check_against(out, clouds, want, 32, max_vox)


def test_fixed_batch_inside_a_hip_graph():
    """capture ``fixed_batch`` alone, overwrite the sweeps in place, replay: equal to an eager call on the new contents (every clear of
    the call is a kernel, the pointer table a kernel argument: nothing of the first contents survives)"""
    import torch
    from quantv2x_amd.voxelizer import GpuVoxelizer
    vz = GpuVoxelizer(RANGE, VS, 32, 2048)
    sets = [[_cloud(2400, 20 + 3 * k + a, sigma=4.0 + 3 * k) for a in range(3)] for k in range(2)]
    sweeps = _dev(sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            vz.fixed_batch(sweeps, 1024)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = vz.fixed_batch(sweeps, 1024)
    counts = []
    for k in (1, 0, 1):
        for s, c in zip(sweeps, sets[k]):
            s.copy_(torch.from_numpy(c))
        graph.replay()
        torch.cuda.synchronize()
        got = {key: out[key].clone() for key in KEYS}
        want = GpuVoxelizer(RANGE, VS, 32, 2048).fixed_batch(_dev(sets[k]), 1024)
        for key in KEYS:
            assert torch.equal(got[key], want[key]), (k, key)
        counts.append(got["voxel_counts"].tolist())
    assert counts[0] != counts[1] and counts[0] == counts[2]
