"""GPU pre-step: LiDAR sweeps -> the ``inputs_m1`` dict of the model.

Replaces ``SpVoxelPreprocessor.preprocess`` + ``collate_batch`` (``pre_processor/sp_voxel_preprocessor.py:54-85,109-174``)
for the deployed path: the points stay on the device, ``qv2x_voxelize_f32`` builds the padded pillars.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import lib as L


class GpuVoxelizer:
    def __init__(self, lidar_range: Sequence[float], voxel_size: Sequence[float], max_points: int = 32,
                 max_voxels: int = 70000, device="cuda"):
        self.lib = L.load()
        self.range = (C.c_float * 6)(*[float(v) for v in lidar_range])
        self.vsize = (C.c_float * 3)(*[float(v) for v in voxel_size])
        self.max_points, self.max_voxels = int(max_points), int(max_voxels)
        self.dev = torch.device(device)
        self._ws = None

    def _outputs(self, rows: int, n: int) -> dict:
        """the four outputs of a call: ``rows`` pillar rows in all, ``n`` voxel counts"""
        return {"voxel_features": torch.empty((rows, self.max_points, 4), dtype=torch.float32, device=self.dev),
                "voxel_coords": torch.empty((rows, 4), dtype=torch.int32, device=self.dev),
                "voxel_num_points": torch.empty((rows,), dtype=torch.int32, device=self.dev),
                "voxel_counts": torch.zeros(n, dtype=torch.int32, device=self.dev)}

    def _workspace(self, need: int, query: str) -> int:
        """the workspace pointer, grown to ``need`` bytes (a negative ``need`` is ``query``'s refusal)"""
        if need < 0:
            L.check(-1, query)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return L.ptr(self._ws)

    def _sweep(self, pts: torch.Tensor, agent: int, capacity: int, need: int, o: dict, row: int, slot: int):
        """one ``qv2x_voxelize_f32`` call: sweep ``pts`` into the ``capacity`` rows of ``o`` from ``row`` on, its count into slot ``slot``"""
        L.check(self.lib.qv2x_voxelize_f32(L.ptr(pts), int(pts.shape[0]), self.range, self.vsize, agent, self.max_points, capacity,
                                           self._workspace(need, "qv2x_voxelize_workspace_bytes"), need, L.ptr(o["voxel_features"][row:]),
                                           L.ptr(o["voxel_coords"][row:]), L.ptr(o["voxel_num_points"][row:]),
                                           L.ptr(o["voxel_counts"][slot:]), L.current_stream()), "qv2x_voxelize_f32")

    def one(self, points: torch.Tensor, agent: int):
        """points f32 [P, 4] on the device -> (voxel_features [M,32,4], voxel_coords [M,4] (agent,z,y,x), voxel_num_points [M])"""
        points = points.contiguous()
        p = int(points.shape[0])
        o = self._outputs(self.max_voxels if p else 0, 1)
        if p == 0:                       # an empty sweep: no pillar (the contract oracle returns empty arrays too)
            return o["voxel_features"], o["voxel_coords"], o["voxel_num_points"]
        self._sweep(points, agent, self.max_voxels, int(self.lib.qv2x_voxelize_workspace_bytes(p)), o, 0, 0)
        m = int(o["voxel_counts"].item())            # the one host sync of the pre-step: the pillar count sizes every later launch
        return o["voxel_features"][:m], o["voxel_coords"][:m], o["voxel_num_points"][:m]

    def fixed(self, sweeps: Sequence[torch.Tensor], capacity: int) -> dict:
        """HIP-graph capturable form: one sweep per batch index, EVERY sweep's ``capacity`` rows handed on (rows past a sweep's voxel count
        carry batch index -1, which the PFN kernel drops), no host read-back.  The returned dict also holds ``voxel_counts`` i32 [n] on
        the device.  Sweeps must keep their point counts between replays of a captured graph.  One ``qv2x_voxelize_f32`` call per sweep."""
        o = self._outputs(len(sweeps) * capacity, len(sweeps))
        need = max(int(self.lib.qv2x_voxelize_workspace_bytes(int(p.shape[0]))) for p in sweeps)
        for a, pts in enumerate(sweeps):
            self._sweep(pts.contiguous(), a, capacity, need, o, a * capacity, a)
        return o

    def fixed_batch(self, sweeps: Sequence[torch.Tensor], capacity: int, first_agent: int = 0) -> dict:
        """``fixed`` from ONE ``qv2x_voxelize_batch_f32`` call (1..64 sweeps, one radix sort over all their points): the same dict, bit for
        bit, with a launch count that does not grow with the number of sweeps.  Empty sweeps are allowed.  HIP-graph capturable under the
        same condition: the sweeps keep their point counts (and their storage) between replays."""
        n = len(sweeps)
        sweeps = [p.contiguous() for p in sweeps]
        o = self._outputs(n * capacity, n)
        npts = (C.c_int32 * n)(*[int(p.shape[0]) for p in sweeps])
        table = (C.c_void_p * n)(*[p.data_ptr() if p.shape[0] else None for p in sweeps])
        need = int(self.lib.qv2x_voxelize_batch_workspace_bytes(n, npts))
        L.check(self.lib.qv2x_voxelize_batch_f32(table, npts, n, self.range, self.vsize, first_agent, self.max_points, capacity,
                                                 self._workspace(need, "qv2x_voxelize_batch_workspace_bytes"), need, L.ptr(o["voxel_features"]),
                                                 L.ptr(o["voxel_coords"]), L.ptr(o["voxel_num_points"]), L.ptr(o["voxel_counts"]),
                                                 L.current_stream()), "qv2x_voxelize_batch_f32")
        return o

    def __call__(self, sweeps: Sequence[torch.Tensor]) -> dict:
        """One sweep per agent -> ``inputs_m1``; agents are the batch index, as ``collate_batch`` does."""
        parts = [self.one(pts, a) for a, pts in enumerate(sweeps)]
        return {"voxel_features": torch.cat([p[0] for p in parts]),
                "voxel_coords": torch.cat([p[1] for p in parts]),
                "voxel_num_points": torch.cat([p[2] for p in parts])}
