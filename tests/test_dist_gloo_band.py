"""The sharded post stage (``ego_only=True, shard_post=True``) on CPU with the gloo backend: every rank computes its row band of ego 0's
view, a second fixed-size all-gather collects the bands, rank 0 assembles them.  The stand-in engine is the CPU oracle of
``test_dist_gloo.py`` with a band method that slices the oracle's whole-map result, so what is under test is the driver: which rows and
ego it asks of each rank, the slab layout on the second link, the assembly, and that the unsharded modes are untouched."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _common import calibrated_plugin, scene_np
from test_dist_gloo import _OracleEngine, _free_port


class _BandOracleEngine(_OracleEngine):
    def __init__(self, state):
        super().__init__(state)
        self.band_calls = []

    def band_shape(self):
        if not hasattr(self, "cout"):
            fused = np.zeros((1, self.h, self.w, 256), np.float32)
            self.cout = int(np.concatenate(self.orc.heads(fused), axis=1).shape[1])
        return self.cout, self.h, self.w

    def head_wire_supported(self, wire):
        return wire == "f32"

    def fuse_frames_and_heads_band(self, gathered, agent_stride, level_stride, frame_stride, pairwise, n_agents, ego, frames, y0, y1, out_slab, wire="f32"):
        self.band_calls.append((y0, y1, ego, n_agents, wire))
        n_calls = len(self.calls)
        full = self.fuse_frames_and_heads(gathered, agent_stride, level_stride, frame_stride, pairwise, n_agents, ego, None, frames)["preds_tensor"]
        del self.calls[n_calls:]                                     # (the whole-map call above is this stand-in's arithmetic, not the driver's)
        band = full[:, :, y0:y1].contiguous().view(-1).view(torch.uint8)
        out_slab[:band.numel()].copy_(band)

    def band_output(self, preds, own_codes, frames):
        return {"preds_tensor": preds.clone()}


def _worker(rank, world, port, state, out_q, frames):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from quantv2x_amd import synth
        from quantv2x_amd.dist import AgentShardedModel
        torch.set_num_threads(1)
        parts = []
        for f in range(frames):
            sc = scene_np(world, seed=3 + f)
            mine = sc["inputs_m1"]["voxel_coords"][:, 0] == rank
            part = {k: v[mine].copy() for k, v in sc["inputs_m1"].items()}
            part["voxel_coords"][:, 0] = f
            parts.append(part)
        inp = {k: torch.from_numpy(np.concatenate([p[k] for p in parts])) for k in parts[0]}
        pose = torch.from_numpy(synth.agent_poses(world, "line")[rank])
        eng = _BandOracleEngine(state)
        own_view = AgentShardedModel(eng, frames=frames).forward(inp, pose)["preds_tensor"].numpy().copy()
        ego_only = AgentShardedModel(eng, ego_only=True, frames=frames).forward(inp, pose)
        calls = list(eng.calls)
        assert not eng.band_calls                                               # the unsharded modes never ask for a band
        model = AgentShardedModel(eng, ego_only=True, shard_post=True, frames=frames)
        banded = model.forward(inp, pose)
        assert eng.calls == calls                                               # ... and the banded one never for a whole map
        # the unsharded modes called again in the same worker, after the banded step: unchanged
        again = AgentShardedModel(eng, ego_only=True, frames=frames).forward(inp, pose)
        assert (again is None) == (rank != 0) and (again is None or torch.equal(again["preds_tensor"], ego_only["preds_tensor"]))
        assert np.array_equal(AgentShardedModel(eng, frames=frames).forward(inp, pose)["preds_tensor"].numpy(), own_view)
        out_q.put((rank, None if banded is None else banded["preds_tensor"].numpy(), None if ego_only is None else ego_only["preds_tensor"].numpy(),
                   list(eng.band_calls), model.gathered_slabs.numpy().copy(), model.slab.numpy().copy()))
    finally:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("world,frames", [(2, 1), (3, 1), (2, 2), (4, 1), (8, 1)])
def test_banded_post_stage_matches_unsharded_ego_only(world, frames):
    from quantv2x_amd.dist import band_payload_layout, band_rows
    from quantv2x_amd.ptq_state import export_ptq_state
    from oracle.spec import Oracle
    state = export_ptq_state(calibrated_plugin())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, state, q, frames)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=600) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    orc = Oracle(state)
    want = np.concatenate([orc.forward(scene_np(world, seed=3 + f), {})["preds_tensor"] for f in range(frames)])
    _, cout, h, w = want.shape
    cap, slab_bytes = band_payload_layout(frames, cout, h, w, world, "f32")
    banded0, ego0 = results[0][1], results[0][2]
    np.testing.assert_array_equal(banded0, ego0)                                # rank 0: the unsharded ego_only output, exactly
    np.testing.assert_allclose(banded0, want, rtol=1e-5, atol=1e-6)             # ... and the single-process oracle (test_dist_gloo.py's bound)
    for rank, banded, _, band_calls, gathered_slabs, slab in results:
        assert (banded is None) == (rank != 0)
        y0, y1 = band_rows(h, world, rank)
        assert band_calls == [(y0, y1, 0, world, "f32")]                        # one band call: its own rows, of ego 0's view
        assert slab.shape == (slab_bytes,) and gathered_slabs.shape == (world, slab_bytes)
        np.testing.assert_array_equal(gathered_slabs[rank], slab)
        for r in range(world):                                                   # the fixed layout: compact [frames][cout][n_cells_r], then padding
            r0, r1 = band_rows(h, world, r)
            n = frames * cout * (r1 - r0) * w
            assert (r1 - r0) * w <= cap
            got = gathered_slabs[r, :4 * n].copy().view(np.float32).reshape(frames, cout, r1 - r0, w)
            np.testing.assert_array_equal(got, ego0[:, :, r0:r1])
