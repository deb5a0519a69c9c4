"""Shared by tests/test_camera_pyramid_cpu.py and tests/test_hip_camera_pyramid.py (no tests here): the tiny Pyramid hypes with a camera
modality ``m2`` next to (or instead of) the LiDAR modality ``m1``, camera inputs, and the calibrated W8A8 mirror model built from them.
The camera grid is 40 x 40 cells of 0.4 m over +-8 m: 20 x 20 behind the backbone's stride 2, against the tiny LiDAR map of 16 x 32 -- the
camera map is cropped in H and padded in W at once (ratios 0.8 and 1.6)."""
import copy

import numpy as np
import torch

CAM_GRID = {"xbound": [-8.0, 8.0, 0.4], "ybound": [-8.0, 8.0, 0.4], "zbound": [-3.0, 3.0, 6.0], "ddiscr": [2.0, 10.0, 8.0], "mode": "LID"}


def camera_hypes(depth_supervision=False, codebook=False, modalities=("m1", "m2")):
    from quantv2x_amd import synth
    hy = synth.make_pyramid_hypes("tiny", codebook=codebook, modalities=modalities)
    hy["model"]["args"]["m2"] = {
        "core_method": "lift_splat_shoot", "sensor_type": "camera",
        "encoder_args": {"grid_conf": dict(CAM_GRID), "data_aug_conf": {"final_dim": (32, 48)}, "img_downsample": 8, "img_features": 16,
                         "camera_encoder": "Resnet101", "use_depth_gt": False, "depth_supervision": depth_supervision},
        "camera_mask_args": {"cav_lidar_range": list(hy["model"]["args"]["lidar_range"]), "grid_conf": dict(CAM_GRID)},
        "backbone_args": {"layer_nums": [2], "layer_strides": [2], "num_filters": [64], "inplanes": 16},
        "aligner_args": {"core_method": "identity"},
    }
    return hy


def camera_inputs(n, views=2, seed=0):
    """RGB-D images (the fourth channel a depth in metres: ``depth_supervision`` reads it), one rig looking ahead"""
    rng = np.random.default_rng(seed)
    imgs = rng.standard_normal((n, views, 4, 32, 48)).astype(np.float32)
    imgs[:, :, 3] = rng.uniform(2.0, 10.0, size=(n, views, 32, 48)).astype(np.float32)
    k = np.array([[30.0, 0.0, 24.0], [0.0, 30.0, 16.0], [0.0, 0.0, 1.0]], np.float32)
    cam_to_ego = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]], np.float32)
    eye = np.eye(3, dtype=np.float32)
    return {"imgs": torch.from_numpy(imgs),
            "rots": torch.from_numpy(np.broadcast_to(cam_to_ego, (n, views, 3, 3)).copy()),
            "trans": torch.from_numpy(np.tile(np.array([0.5, 0.0, 1.5], np.float32), (n, views, 1))),
            "intrins": torch.from_numpy(np.broadcast_to(k, (n, views, 3, 3)).copy()),
            "post_rots": torch.from_numpy(np.broadcast_to(eye, (n, views, 3, 3)).copy()),
            "post_trans": torch.zeros(n, views, 3)}


def camera_scene(agents, seed=3, device="cpu"):
    """a tiny scene whose agents have the modalities ``agents``; the camera agents' ``inputs_m2`` are images"""
    from quantv2x_amd import synth
    dd = synth.scene_to_torch(synth.make_scene("tiny", n_agents=len(agents), seed=seed, n_points=3000, modalities=list(agents)), device)
    k = sum(a == "m2" for a in agents)
    if k:
        dd["inputs_m2"] = {name: t.to(device) for name, t in camera_inputs(k, seed=seed).items()}
    return dd


def calibrated_camera_model(codebook=False, modalities=("m1", "m2"), agents=("m1", "m2", "m2")):
    """W8A8 min-max, one EMA pass, frozen: the recipe of ``_common.calibrated_pyramid_plugin`` on the model with a camera modality"""
    from _common import quant_wrap
    from quantv2x_amd import synth
    from quantv2x_amd.plugin.tools import train_utils
    from quantv2x_amd.plugin.tools.inference_quant import calibrate_minmax
    model = train_utils.create_model(copy.deepcopy(camera_hypes(codebook=codebook, modalities=modalities))).eval()
    synth.load_state_dict_numpy(model, synth.make_state_dict(model.state_dict(), seed=1))
    return calibrate_minmax(quant_wrap(model), [camera_scene(list(agents))])
