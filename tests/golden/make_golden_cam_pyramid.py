"""tests/golden/cam_pyramid.npz: the reference's own, unmodified ``PyramidFusion`` (opencood/models/fuse_modules/pyramid_fuse.py:64-167, fp32,
eval mode, ``stage: collab``) with camera agents in the scene -- the crop mask it puts on their fusion scores at every level (:147-162).

The model is the fusion backbone of the tiny Pyramid hypes (ResNeXt levels 64 / 128 / 256 at 16 x 32, 8 x 16, 4 x 8) with
``synth.make_state_dict`` weights (seeded per key, so the mirror's state dict gets the same values).  Input: seeded features
[3, 64, 16, 32] on a 1/64 grid (stored as int16 ``x_q``, x = x_q / 64), ``record_len [3]``, three agents on a ring (rotations and
translations).  Two cases, one per ratio pair:
  a  agent modalities [m1, m2, m2], crop ratios (H, W) = (0.8, 1.6)
  b  agent modalities [m2, m1, m2], crop ratios (6.4 / 9.6, 12.8 / 9.6): at level 0 the rectangle's first row is -1, which the reference's
     slice wraps; at level 2 both rectangles are empty and the camera agents' scores are zero everywhere
Stored per case (prefix ``a/`` | ``b/``): ``modalities``, ``ratio_H``, ``ratio_W`` (float64), per level ``occ{i}`` (the occupancy map
[3, 1, h, w] of ``occ_outputs``) and ``score{i}`` (the score as it enters ``weighted_fuse``, recorded by wrapping that function), and
``fused`` = every fourth channel of the fused output [1, 96, 16, 32].  Shared: ``x_q``, ``pairwise``, ``affine``, ``HW_metres``, ``seed_w``.

Run on one thread, as make_golden.py (bit-reproducible reductions); the test pins the same.  Between one and eight threads 35 of the 49 152
stored fused values of case a moved by up to 4e-3 (measured with the mirror), more than the test's tolerance; the scores and occupancy maps did not.

Needs the reference tree at ``/root/reference``, which ``_refimport`` imports on the CPU: ``python tests/golden/make_golden_cam_pyramid.py``."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(os.path.dirname(HERE))]
import _refimport  # noqa: E402

SEED_W, SEED_X = 5, 23
H_METRES, W_METRES = 12.8, 25.6
CASES = {"a": (["m1", "m2", "m2"], 0.8, 1.6), "b": (["m2", "m1", "m2"], 6.4 / 9.6, 12.8 / 9.6)}


def features():
    g = np.random.Generator(np.random.PCG64(SEED_X))
    return np.clip(np.rint(g.standard_normal((3, 64, 16, 32)) * 64.0), -32000, 32000).astype(np.int16)


def main():
    _refimport.install()
    import torch
    torch.set_num_threads(1)           # single thread, as make_golden.py: bit-reproducible reductions (the tests set the same)
    from opencood.models.fuse_modules import pyramid_fuse as ref
    from opencood.utils.transformation_utils import normalize_pairwise_tfm
    from quantv2x_amd import synth

    cfg = copy.deepcopy(synth.make_pyramid_hypes("tiny")["model"]["args"]["fusion_backbone"])
    model = ref.PyramidFusion(cfg).eval()
    synth.load_state_dict_numpy(model, synth.make_state_dict(model.state_dict(), seed=SEED_W))
    x_q = features()
    x = torch.from_numpy(x_q.astype(np.float32) / np.float32(64.0))
    pw = torch.from_numpy(synth.pairwise_t_matrix(synth.agent_poses(3, "ring"), 5)[None])
    affine = normalize_pairwise_tfm(pw.clone(), H_METRES, W_METRES, 1)
    out = {"x_q": x_q, "pairwise": pw.numpy(), "affine": affine.numpy(), "HW_metres": np.array([H_METRES, W_METRES]), "seed_w": np.int64(SEED_W)}

    scores = []
    inner = ref.weighted_fuse

    def recording(xx, score, *a, **k):
        scores.append(score.detach().clone().numpy())
        return inner(xx, score, *a, **k)
    ref.weighted_fuse = recording
    try:
        for tag, (mods, rh, rw) in CASES.items():
            del scores[:]
            info = {"m2": {"crop_ratio_W_m2": rw, "crop_ratio_H_m2": rh}}
            with torch.no_grad():
                fused, occ = model(x, torch.tensor([3]), affine, mods, info)
            assert len(scores) == len(occ) == 3
            out[f"{tag}/modalities"], out[f"{tag}/ratio_H"], out[f"{tag}/ratio_W"] = np.array(mods), np.float64(rh), np.float64(rw)
            for i in range(3):
                out[f"{tag}/occ{i}"], out[f"{tag}/score{i}"] = occ[i].numpy(), scores[i]
                cam = [j for j, m in enumerate(mods) if m == "m2"]
                print(tag, "level", i, "zero share of the camera agents' scores:", float((scores[i][cam] == 0).mean()))
            out[f"{tag}/fused"] = fused.numpy()[:, ::4].copy()
    finally:
        ref.weighted_fuse = inner
    path = os.path.join(HERE, "cam_pyramid.npz")
    np.savez_compressed(path, **out)
    print("cam_pyramid.npz", os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
