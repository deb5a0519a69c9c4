"""LiDAR sweeps -> boxes for a batch of single-agent frames, three calls around the model: ``qv2x_voxelize_batch_f32`` (all sweeps, one
radix sort), the deployed engine, ``qv2x_postprocess_batch_f32`` (all frames, the frame a grid dimension).  Nothing is read back on the
way, so the chain replays as one HIP graph.  Scenes of several agents are out of scope here (the voxelizer entry supports them through
``first_agent``; the post-process of a fused scene is one frame).  Both post-processors of the reference's yamls are accepted: the multi-class
``VoxelPostprocessor3Heads`` and the single-class ``VoxelPostprocessor``."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from .engine import capture_call
from .plugin.data_utils.post_processor.voxel_postprocessor import gpu_post_process_batch
from .voxelizer import GpuVoxelizer


class PointsToBoxes:
    def __init__(self, engine, voxelizer: GpuVoxelizer, postprocessor, capacity: int, max_boxes: int = 1000):
        """``engine``: a deployed model (``quantv2x_amd.engine.deploy``); ``postprocessor``: the post-processor of the model's yaml -- the
        multi-class ``VoxelPostprocessor3Heads`` (V2X-Real) or the single-class ``VoxelPostprocessor`` (the OPV2V and DAIR-V2X yamls), each
        with the parameters its own ``post_process`` uses; ``capacity``: pillar rows handed on per sweep (rows past a sweep's voxels carry
        batch index -1)."""
        self.engine, self.voxelizer, self.postprocessor = engine, voxelizer, postprocessor
        self.capacity, self.max_boxes = int(capacity), int(max_boxes)
        anchors = postprocessor.generate_anchor_box()
        self.single_class = not isinstance(anchors, tuple)
        if self.single_class:                            # VoxelPostprocessor.generate_anchor_box: one array (H, W, anchor, 7)
            a = torch.as_tensor(np.asarray(anchors)).to(torch.float32).contiguous()
            self.anchors_dev, self.per_cell = a.reshape(-1, 7).to(voxelizer.dev), int(a.shape[2])
        else:                                            # VoxelPostprocessor3Heads: (anchors per class, anchors per location)
            a = torch.as_tensor(np.array(anchors[0])).to(torch.float32).permute(1, 2, 0, 3, 4).contiguous()    # (H, W, class, anchor, 7)
            self.anchors_dev, self.per_cell = a.reshape(-1, 7).to(voxelizer.dev), int(a.shape[2] * a.shape[3])
        self._fixed = {}                                 # per frame count: what a call needs besides the sweeps, made once (no H2D copy later)

    def _constants(self, frames: int):
        c = self._fixed.get(frames)
        if c is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("PointsToBoxes: first call with this many frames during HIP-graph capture (use capture())")
            dev = self.voxelizer.dev
            c = self._fixed[frames] = (torch.eye(4, dtype=torch.float64).reshape(1, 1, 1, 4, 4).repeat(frames, 5, 5, 1, 1).to(dev),
                                       torch.ones(frames, dtype=torch.int64),
                                       torch.eye(4, dtype=torch.float32).repeat(frames, 1, 1).to(dev).contiguous())
        return c

    def __call__(self, sweeps: Sequence[torch.Tensor], transforms: torch.Tensor = None) -> dict:
        """One sweep (f32 [P, 4] on the device) per frame -> ``corners`` [frames, max_boxes, 8, 3], ``scores`` / ``labels``
        [frames, max_boxes], ``counts`` i32 [frames] (frame f's boxes: the first ``counts[f]`` rows) and ``voxel_counts``, all on the
        device.  ``transforms``: f32 [frames, 4, 4] on the device (default: identity)."""
        frames = len(sweeps)
        pairwise, record_len, eye = self._constants(frames)
        pp = self.postprocessor
        inp = self.voxelizer.fixed_batch(sweeps, self.capacity)
        o = self.engine({"inputs_m1": inp, "agent_modality_list": ["m1"] * frames, "record_len": record_len, "pairwise_t_matrix": pairwise})
        if self.single_class:                            # what VoxelPostprocessor.post_process passes on: the direction head when the model has one
            dirp = o.get("dir_preds")
            has_dir = dirp is not None and dirp.shape[1] > 0
            corners, scores, labels, counts = gpu_post_process_batch(
                pp, o["cls_preds"], o["reg_preds"], dirp if has_dir else None, self.anchors_dev, eye if transforms is None else transforms,
                anchors_per_cell=self.per_cell, num_classes=1, num_bins=int(pp.params["dir_args"]["num_bins"]) if has_dir else 0,
                dir_offset=float(pp.params["dir_args"]["dir_offset"]) if has_dir else 0.0, rng=pp.params["gt_range"], range_xy_only=False,
                max_extent=6.0, z_lim=(-3.0, 1.0), max_boxes=self.max_boxes)
            return {"corners": corners, "scores": scores, "labels": labels, "counts": counts, "voxel_counts": inp["voxel_counts"]}
        corners, scores, labels, counts = gpu_post_process_batch(
            pp, o["cls_preds"], o["reg_preds"], None, self.anchors_dev, eye if transforms is None else transforms,
            anchors_per_cell=self.per_cell, num_classes=int(o["cls_preds"].shape[1] // self.per_cell), num_bins=0, dir_offset=0.0,
            rng=pp.gt_range, range_xy_only=True, max_extent=100.0, z_lim=(-100.0, 100.0), max_boxes=self.max_boxes)
        return {"corners": corners, "scores": scores, "labels": labels, "counts": counts, "voxel_counts": inp["voxel_counts"]}

    def capture(self, sweeps: Sequence[torch.Tensor], transforms: torch.Tensor = None):
        """Capture one call into a HIP graph (``engine.capture_call``: two warm-up calls on a side stream first).  The returned callable
        replays it on the same sweep tensors -- refresh their contents in place between replays, the point counts stay -- and returns the
        same output dict; ``replay.graph`` is the graph."""
        return capture_call(lambda: self(sweeps, transforms))
