"""The ego's post stage in row bands on the GPU (``AgentShardedModel(ego_only=True, shard_post=True)``, ``csrc/fuse_att.hip``,
``csrc/heads_f32.hip``): the band entry points against the whole-map entry points on the same inputs, BIT FOR BIT -- a cell's sampling grid
comes from its global coordinates and its fma / MFMA chain runs over its own row, whichever tile or lane it lands in; the u8 wire carries
the output quantizer's code, whose dequantization is the fp32 output.  The yardstick is the whole-map call (itself checked against the CPU
oracle in test_hip_ego.py / test_hip_fullsize.py), so no tolerance appears here."""
import ctypes as C

import numpy as np
import pytest
import torch

from _common import calibrated_plugin, scene_np

pytestmark = pytest.mark.gpu


def _deploy(state):
    from quantv2x_amd.engine import deploy
    eng = deploy(state=state)
    eng.single_agent_tables = False          # (the band path never takes the single-agent table look-up: another fp32 association)
    return eng


@pytest.fixture(scope="module")
def tiny():
    from quantv2x_amd.ptq_state import export_ptq_state
    state = export_ptq_state(calibrated_plugin("tiny", n_agents=2))
    return state, _deploy(state)


@pytest.fixture(scope="module")
def tiny_max():
    from quantv2x_amd.ptq_state import export_ptq_state
    return _deploy(export_ptq_state(calibrated_plugin("tiny", n_agents=2, fusion="max")))


@pytest.fixture(scope="module")
def v2xreal():
    from test_hip_fullsize import _calibrated
    return _deploy(_calibrated("v2xreal"))


def wire_scene(eng, sc, n, layout, frames=2):
    """The driver's view of ``frames`` scenes of ``n`` agents after the first all-gather: agent-major payloads (code planes
    [levels, frames, hw], then the poses; frame 1 = the agents in reversed wire order) and the pairwise matrices from the gathered poses."""
    from quantv2x_amd import synth
    from quantv2x_amd.dist import POSE_BYTES, payload_layout
    taps = {}
    eng(synth.scene_to_torch(sc, "cuda"), taps)
    hw = eng.fh * eng.fw
    codes_np = taps["codes"].clone().view(eng.levels, n, hw).cpu().numpy()
    cbytes, pose_off, pbytes = payload_layout(eng.levels, frames, hw)
    poses = synth.agent_poses(n, layout)
    gathered = torch.zeros((n, pbytes), dtype=torch.uint8, device="cuda")
    per_frame = [codes_np, codes_np[:, ::-1].copy()]
    for a in range(n):
        planes = np.stack([per_frame[f % 2][:, a] for f in range(frames)], axis=1)
        gathered[a, :cbytes] = torch.from_numpy(planes.reshape(-1)).cuda()
        gathered[a, pose_off:] = torch.from_numpy(np.tile(poses[a].reshape(-1), frames).view(np.uint8)).cuda()
    L_ = sc["pairwise_t_matrix"].shape[1]
    pairwise = torch.zeros((frames, L_, L_, 4, 4), dtype=torch.float64, device="cuda")
    eng.pairwise_frames_from_poses(gathered, n, pbytes, pose_off, frames, POSE_BYTES, L_, pairwise)
    return gathered, pbytes, pairwise


def whole_map(eng, gathered, pbytes, pairwise, n, ego, frames):
    hw = eng.fh * eng.fw
    out = eng.fuse_frames_and_heads(gathered, pbytes, frames * hw, hw, pairwise, n, ego, None, frames)["preds_tensor"].clone()
    torch.cuda.synchronize()
    return out


def band_values(eng, slab, frames, rows, wire):
    """a band slab -> its fp32 values [frames, cout, rows, W] (the u8 wire dequantized as the receiver does)"""
    hd, n = eng.heads, frames * eng.heads.cout * rows * eng.fw
    if wire == "f32":
        return slab[:4 * n].view(torch.float32).view(frames, hd.cout, rows, eng.fw)
    codes = slab[:n].view(frames, hd.cout, rows, eng.fw).to(torch.float32)
    return (codes - hd.za[:hd.cout].view(1, -1, 1, 1)) * hd.da[:hd.cout].view(1, -1, 1, 1)


def check_bands(eng, sc, n, layout, worlds=(2, 3, 8), egos=(0, 1), frames=2):
    from quantv2x_amd.dist import band_payload_layout, band_rows
    gathered, pbytes, pairwise = wire_scene(eng, sc, n, layout, frames)
    hd, h, w, hw = eng.heads, eng.fh, eng.fw, eng.fh * eng.fw
    assert eng.head_wire_supported("u8")
    try:
        for ego in egos:
            full = whole_map(eng, gathered, pbytes, pairwise, n, ego, frames)
            for world in worlds:
                for wire in ("f32", "u8"):
                    _, slab_bytes = band_payload_layout(frames, hd.cout, h, w, world, wire)
                    slabs = torch.full((world, slab_bytes), 0xA5, dtype=torch.uint8, device="cuda")
                    for one_launch in (True, False):                       # every kernel form the band path can select
                        eng.band_one_launch = one_launch
                        slabs.fill_(0xA5)
                        for r in range(world):
                            y0, y1 = band_rows(h, world, r)
                            eng.fuse_frames_and_heads_band(gathered, pbytes, frames * hw, hw, pairwise, n, ego, frames, y0, y1, slabs[r], wire)
                            got = band_values(eng, slabs[r], frames, y1 - y0, wire)
                            assert torch.equal(got, full[:, :, y0:y1]), (ego, world, wire, one_launch, r)
                        # (b) the union of the bands through the HIP assemble kernel = the whole-map predictions, = the plain-torch assembly
                        from quantv2x_amd.dist import assemble_bands_reference
                        out = torch.full((frames, hd.cout, h, w), float("nan"), dtype=torch.float32, device="cuda")
                        eng.assemble_bands(slabs, world, frames, wire, out)
                        torch.cuda.synchronize()
                        assert torch.equal(out, full), (ego, world, wire, one_launch)
                        ref = assemble_bands_reference(slabs, frames, hd.cout, h, w, world, wire, hd.da[:hd.cout], hd.za[:hd.cout])
                        assert torch.equal(out, ref)
    finally:
        eng.band_one_launch = None


@pytest.mark.parametrize("n_agents,layout", [(3, "line"), (8, "line")])
def test_tiny_bands_equal_the_whole_map_call(tiny, n_agents, layout):
    _, eng = tiny
    check_bands(eng, scene_np(n_agents, seed=9), n_agents, layout)     # (cell ranges off the 32-cell tiles: test_band_entry_points_on_any_cell_range)


def test_tiny_bands_max_fusion(tiny_max):
    check_bands(tiny_max, scene_np(3, seed=4), 3, "line", worlds=(3,))


def test_v2xreal_four_agents_bands_equal_the_whole_map_call(v2xreal):
    from quantv2x_amd import synth
    sc = synth.make_scene("v2xreal", n_agents=4, seed=5, n_points=60000, layout="ring")
    check_bands(v2xreal, sc, 4, "ring", egos=(0, 2))


@pytest.mark.parametrize("cell0,n_cells", [(0, None), (37, 45), (5, 1), (None, 33), (64, 96)])
def test_band_entry_points_on_any_cell_range(tiny, cell0, n_cells):
    """The C entry points themselves on ranges that are no row bands: a ``cell0`` off every multiple of 32, a ragged last tile, one cell,
    the map's last cells, the whole map -- fused rows, heads on them and the one-launch form, both wires, three scenes in a launch."""
    from quantv2x_amd import lib as L
    _, eng = tiny
    n, frames = 3, 3
    gathered, pbytes, pairwise = wire_scene(eng, scene_np(n, seed=9), n, "line", frames)
    hd, hw = eng.heads, eng.fh * eng.fw
    n_cells = hw if n_cells is None else n_cells
    cell0 = hw - n_cells if cell0 is None else cell0
    offsets, lens = [f * hw for f in range(frames)], [n] * frames
    fused_full = torch.empty((frames, hw, 256), dtype=torch.float32, device="cuda")
    eng.fuse_scenes(L.ptr(gathered), pbytes, frames * hw, None, pairwise, offsets, lens, fused_full, 1)
    full = whole_map(eng, gathered, pbytes, pairwise, n, 1, frames).view(frames, hd.cout, hw)
    d = eng._fuse_desc(pbytes, frames * hw, pairwise[0], n, 1)
    offs, cnts = (C.c_int64 * frames)(*offsets), (C.c_int32 * frames)(*lens)
    st = L.current_stream()
    rows = torch.full((frames, n_cells, 256), float("nan"), dtype=torch.float32, device="cuda")
    L.check(eng.lib.qv2x_fuse_att_band_f32(C.byref(d), frames, offs, cnts, L.ptr(gathered), L.ptr(eng.lut), L.ptr(eng.lut_bias), None, L.ptr(pairwise),
                                           cell0, n_cells, L.ptr(rows), st))
    torch.cuda.synchronize()
    assert torch.equal(rows, fused_full[:, cell0:cell0 + n_cells])
    for wire, dtype in (("f32", torch.float32), ("u8", torch.uint8)):
        def values(t):
            return t if wire == "f32" else (t.to(torch.float32) - hd.za[:hd.cout].view(1, -1, 1)) * hd.da[:hd.cout].view(1, -1, 1)
        out = torch.zeros((frames, hd.cout, n_cells), dtype=dtype, device="cuda")
        L.check(eng.lib.qv2x_heads_band(L.ptr(rows), frames, n_cells, hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da), L.ptr(hd.za),
                                        L.WIRES[wire], L.ptr(hd.da_np), L.ptr(out), st))
        tap = torch.full((frames, n_cells, 256), float("nan"), dtype=torch.float32, device="cuda")
        one = torch.zeros((frames, hd.cout, n_cells), dtype=dtype, device="cuda")
        L.check(eng.lib.qv2x_fuse_heads_band(C.byref(d), frames, offs, cnts, L.ptr(gathered), L.ptr(eng.lut), L.ptr(eng.lut_bias), None, L.ptr(pairwise),
                                             cell0, n_cells, hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da), L.ptr(hd.za),
                                             L.WIRES[wire], L.ptr(hd.da_np), L.ptr(one), L.ptr(tap), st))
        torch.cuda.synchronize()
        assert torch.equal(values(out), full[:, :, cell0:cell0 + n_cells]), wire
        assert torch.equal(values(one), full[:, :, cell0:cell0 + n_cells]), wire
        assert torch.equal(tap, rows)


def test_refusals_leave_the_process_running(tiny):
    """(c) the u8 wire without a quantizer on every channel, and ranges outside the map: QV2X_EINVAL with a message, no launch"""
    from quantv2x_amd import lib as L
    from quantv2x_amd.dist import AgentShardedModel
    state, eng = tiny
    off = dict(state)
    off["dir_head/a_off"] = np.bool_(True)
    eng_off = _deploy(off)
    assert eng.head_wire_supported("u8") and eng_off.head_wire_supported("f32") and not eng_off.head_wire_supported("u8")
    with pytest.raises(ValueError):
        eng.head_wire_supported("f16")
    with pytest.raises(ValueError, match="cannot serve"):
        AgentShardedModel(eng_off, ego_only=True, shard_post=True, band_wire="u8")
    n, frames = 3, 1
    gathered, pbytes, pairwise = wire_scene(eng, scene_np(n, seed=9), n, "line", frames)
    hd, hw = eng.heads, eng.fh * eng.fw
    slab = torch.zeros(frames * hd.cout * hw * 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.Qv2xError):
        eng_off.fuse_frames_and_heads_band(gathered, pbytes, frames * hw, hw, pairwise, n, 0, frames, 0, eng.fh, slab, "u8")
    d = eng._fuse_desc(pbytes, frames * hw, pairwise[0], n, 0)
    offs, cnts = (C.c_int64 * 1)(0), (C.c_int32 * 1)(n)
    st = L.current_stream()
    rows = torch.zeros((hw, 256), dtype=torch.float32, device="cuda")
    mixed = hd.da_np.copy()
    mixed[3] = -1.0

    def one_launch(cell0, n_cells, out=slab, wire="f32", da_host=hd.da_np):
        return eng.lib.qv2x_fuse_heads_band(C.byref(d), 1, offs, cnts, L.ptr(gathered), L.ptr(eng.lut), L.ptr(eng.lut_bias), None, L.ptr(pairwise),
                                            cell0, n_cells, hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da), L.ptr(hd.za),
                                            L.WIRES[wire], L.ptr(da_host), L.ptr(out), None, st)

    def fuse(cell0, n_cells, out=rows):
        return eng.lib.qv2x_fuse_att_band_f32(C.byref(d), 1, offs, cnts, L.ptr(gathered), L.ptr(eng.lut), L.ptr(eng.lut_bias), None, L.ptr(pairwise),
                                              cell0, n_cells, L.ptr(out), st)

    def heads(n_cells, out=slab, wire="f32", da_host=hd.da_np):
        return eng.lib.qv2x_heads_band(L.ptr(rows), 1, n_cells, hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da), L.ptr(hd.za),
                                       L.WIRES[wire], L.ptr(da_host), L.ptr(out), st)
    for call in (one_launch, fuse):
        for bad in ((-1, 4), (0, -1), (0, hw + 1), (hw - 3, 4), (hw + 1, 0), (1 << 40, 1)):
            assert call(*bad) == -1, (call.__name__, bad)
            assert b"map" in eng.lib.qv2x_last_error()
        assert call(0, 4, out=None) == -1 and b"null" in eng.lib.qv2x_last_error()
        assert call(7, 0) == 0 and call(hw, 0) == 0                    # an empty band: QV2X_OK, nothing launched
    assert heads(-1) == -1 and heads(4, out=None) == -1 and heads(0) == 0
    for call in (lambda **kw: one_launch(0, 4, **kw), lambda **kw: heads(4, **kw)):
        assert call(wire="u8", da_host=mixed) == -1 and b"quantizer" in eng.lib.qv2x_last_error()
        assert call(wire="u8", da_host=None) == -1
        assert call(wire="u8") == 0
    assert eng.lib.qv2x_fuse_heads_band(C.byref(d), 1, offs, cnts, L.ptr(gathered), L.ptr(eng.lut), L.ptr(eng.lut_bias), None, L.ptr(pairwise), 0, 4,
                                        hd.cout, hd.cout_pad, L.ptr(hd.w), L.ptr(hd.bias), L.ptr(hd.da), L.ptr(hd.za), 2, L.ptr(hd.da_np), L.ptr(slab), None, st) == -1
    out = torch.zeros((1, hd.cout, eng.fh, eng.fw), dtype=torch.float32, device="cuda")
    asm = eng.lib.qv2x_assemble_bands
    ok = (L.ptr(slab), 1, slab.numel(), 1, hd.cout, eng.fh, eng.fw, 0, L.ptr(hd.da), L.ptr(hd.za), L.ptr(out), st)
    assert asm(*ok) == 0
    for i, v in ((0, None), (10, None), (1, 0), (2, slab.numel() - 16), (2, slab.numel() + 8), (7, 2), (3, 70000)):
        bad = list(ok)
        bad[i] = v
        assert asm(*bad) == -1, (i, v)
    bad = list(ok)
    bad[7], bad[8] = 1, None
    assert asm(*bad) == -1                                               # the u8 wire dequantizes: it needs da and za
    assert asm(C.c_void_p(slab.data_ptr() + 4), 1, slab.numel() - 16, 1, hd.cout, eng.fh, eng.fw, 1, L.ptr(hd.da), L.ptr(hd.za), L.ptr(out), st) == -2
    # the process continues: a whole band after all that
    full = whole_map(eng, gathered, pbytes, pairwise, n, 0, frames)
    eng.fuse_frames_and_heads_band(gathered, pbytes, frames * hw, hw, pairwise, n, 0, frames, 0, eng.fh, slab, "f32")
    assert torch.equal(band_values(eng, slab, frames, eng.fh, "f32"), full)


def _own_frames(frames, seeds):
    """this rank's agent of `frames` single-agent frames, padded to a fixed pillar count (unused rows: agent index -1)"""
    parts = []
    for f in range(frames):
        part = {k: v.copy() for k, v in scene_np(1, seed=seeds + f)["inputs_m1"].items()}
        part["voxel_coords"][:, 0] = f
        parts.append(part)
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _padded(a, rows):
    inp = {}
    for k, v in a.items():
        pad = np.zeros((rows - v.shape[0],) + v.shape[1:], v.dtype)
        if k == "voxel_coords":
            pad[:] = -1
        if k == "voxel_num_points":
            pad[:] = 1
        inp[k] = np.concatenate([v, pad])
    return inp


@pytest.mark.parametrize("wire", ["f32", "u8"])
def test_driver_world_one_equals_unsharded_ego_only(tiny, wire):
    """(d) one rank, graphs on: the banded step (pre | band | assemble around the two exchanges) gives the unsharded ``ego_only`` output bit
    for bit, the ``*_single`` keys included, also when the captured graphs are replayed on refreshed inputs."""
    from quantv2x_amd import synth
    from quantv2x_amd.dist import AgentShardedModel
    _, eng = tiny
    frames = 2
    a, b = _own_frames(frames, 3), _own_frames(frames, 11)
    rows = max(a["voxel_features"].shape[0], b["voxel_features"].shape[0])
    a, b = _padded(a, rows), _padded(b, rows)
    inp = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    poses = torch.from_numpy(np.stack(synth.agent_poses(1, "line"))).cuda()
    kw = dict(frames=frames, max_cav=5, emulate_world=1, emulate_poses=poses, ego_only=True, graphs=True)
    plain = AgentShardedModel(eng, **kw)
    banded = AgentShardedModel(eng, shard_post=True, band_wire=wire, **kw)
    for step, src in enumerate((a, b, a)):
        for k, v in src.items():
            inp[k].copy_(torch.from_numpy(v))                          # refreshed in place: the graphs are replayed, not re-captured
        want = {k: v.clone() for k, v in plain.forward(inp, poses[0]).items()}
        got = banded.forward(inp, poses[0])
        torch.cuda.synchronize()
        assert sorted(got) == sorted(want) and any(k.endswith("_single") for k in want)
        for k in want:
            assert torch.equal(got[k], want[k]), (step, k)
        if step == 0:
            graphs = banded._captured[1:4]
            first = want["preds_tensor"]
        assert banded._captured[1:4] == graphs and all(g is not None for g in graphs)
    assert not torch.equal(first, plain.forward({k: torch.from_numpy(v).cuda() for k, v in b.items()}, poses[0])["preds_tensor"])   # (the refresh did change the scene)


@pytest.mark.parametrize("rank", [0, 7])
def test_rehearsal_of_a_world_of_eight(tiny, rank):
    """(e) one process plays rank r of eight: capture and replay run; its slab is rows band_rows(h, 8, r) of the whole-map call on the same
    gathered buffer.  (The assembled map of a rehearsal is not a scene output: every slot holds this rank's band.)"""
    from quantv2x_amd import synth
    from quantv2x_amd.dist import AgentShardedModel, band_rows
    _, eng = tiny
    frames, W = 2, 8
    inp = {k: torch.from_numpy(v).cuda() for k, v in _own_frames(frames, 3).items()}
    poses = torch.from_numpy(np.stack(synth.agent_poses(W, "ring"))).cuda()
    for wire in ("f32", "u8"):
        sh = AgentShardedModel(eng, frames=frames, max_cav=8, emulate_world=W, emulate_poses=poses, emulate_rank=rank, ego_only=True, shard_post=True,
                               band_wire=wire, graphs=True)
        out = sh.forward(inp, poses[rank])
        out = sh.forward(inp, poses[rank])                               # the replay
        torch.cuda.synchronize()
        assert (out is None) == (rank != 0)
        pre, band, asm = sh.stage_graphs()
        assert pre is not None and band is not None and (asm is None) == (rank != 0)
        hw = eng.fh * eng.fw
        full = whole_map(eng, sh.gathered, sh.payload_bytes, sh.pairwise, W, 0, frames)
        y0, y1 = band_rows(eng.fh, W, rank)
        assert torch.equal(band_values(eng, sh.slab, frames, y1 - y0, wire), full[:, :, y0:y1]), wire
        if rank == 0:
            assert out["preds_tensor"].shape == full.shape and torch.equal(out["preds_tensor"][:, :, y0:y1], full[:, :, y0:y1])
