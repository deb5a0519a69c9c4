"""Shared by the lift-splat tests: the fixture's scenes (tests/golden/lift_splat.npz, written by tests/golden/make_golden_lss.py from the
reference's own functions) and small synthetic camera rigs for the constructed cases."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lift_splat.npz")
SCENES = ("a", "b", "c")
CAM_TO_EGO = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]], np.float32)   # camera (x right, y down, z ahead) -> ego (x ahead, y left, z up)
MATRICES = ("rots", "trans", "intrins", "post_rots", "post_trans")


@functools.lru_cache(maxsize=None)
def _file():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def scene(name):
    """the arrays of one fixture scene, without the prefix; read-only"""
    out = {k[2:]: v for k, v in _file().items() if k.startswith(name + "_")}
    for v in out.values():
        v.setflags(write=False)
    return out


def grid_conf(s):
    return {"xbound": s["xbound"].tolist(), "ybound": s["ybound"].tolist(), "zbound": s["zbound"].tolist(),
            "ddiscr": [float(s["ddiscr"][0]), float(s["ddiscr"][1]), int(s["ddiscr"][2])], "mode": str(s["mode"])}


def yaw_rot(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return (np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ CAM_TO_EGO).astype(np.float32)


def rig(samples, views, final_dim, seed=0, spread=True):
    """camera matrices f32 [samples, views, ...]: level cameras 1.5 m up at yaws of their own (``spread``) or all looking ahead, a pinhole
    whose focal length is 0.6 of the image width, the identity augmentation"""
    g = np.random.default_rng(seed)
    h, w = final_dim
    m = {"rots": np.zeros((samples, views, 3, 3), np.float32), "trans": np.zeros((samples, views, 3), np.float32),
         "intrins": np.zeros((samples, views, 3, 3), np.float32), "post_rots": np.tile(np.eye(3, dtype=np.float32), (samples, views, 1, 1)),
         "post_trans": np.zeros((samples, views, 3), np.float32)}
    for s in range(samples):
        for v in range(views):
            m["rots"][s, v] = yaw_rot((2 * np.pi * v / views + g.uniform(-0.3, 0.3)) if spread else 0.0)
            m["trans"][s, v] = [g.uniform(-1, 1), g.uniform(-0.5, 0.5), 1.5] if spread else [0.0, 0.0, 1.5]
            m["intrins"][s, v] = [[0.6 * w, 0, w / 2], [0, 0.6 * w, h / 2], [0, 0, 1]]
    return m
