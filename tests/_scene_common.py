"""Shared by the scene-preparation tests: the scene transforms (``world``, ``pairwise``, agent-to-ego) from 6-DoF poses with ``x_to_world`` of
the plugin and the fixed-order ``oracle.geometry.solve4`` -- the arithmetic csrc/solve4.h runs on the device ."""
import numpy as np

from oracle.geometry import solve4
from quantv2x_amd.plugin.utils.transformation_utils import x_to_world


def solve_outputs(world, counts, proj_first=False):
    """``pairwise`` [S, L, L, 4, 4] and ``to_ego`` [S, L, 4, 4] from world matrices [S, L, 4, 4]: solve4 below each scene's (clamped) count,
    identity elsewhere; ``pairwise`` all identity under ``proj_first``"""
    S, L = world.shape[:2]
    pairwise, to_ego = np.tile(np.eye(4), (S, L, L, 1, 1)), np.tile(np.eye(4), (S, L, 1, 1))
    for s in range(S):
        n = int(min(max(int(counts[s]), 0), L))
        for i in range(n):
            for j in range(n):
                if i != j and (j == 0 or not proj_first):
                    x = solve4(world[s, j], world[s, i])
                    if not proj_first:
                        pairwise[s, i, j] = x
                    if j == 0:
                        to_ego[s, i] = x
    return pairwise, to_ego


def statement(poses, counts, proj_first=False):
    """poses [S, L, 6] (x, y, z, roll, yaw, pitch; degrees; agent 0 the ego), counts [S] -> dict ``world`` [S, L, 4, 4], ``pairwise``
    [S, L, L, 4, 4] (``solve(T_j, T_i)``; all identity under ``proj_first``), ``to_ego`` (``solve(T_0, T_a)``) and ``to_ego_f32``; identity in
    the padding"""
    poses = np.asarray(poses, np.float64)
    S, L = poses.shape[:2]
    world = np.tile(np.eye(4), (S, L, 1, 1))
    for s in range(S):
        for a in range(int(min(max(int(counts[s]), 0), L))):
            world[s, a] = x_to_world(poses[s, a])
    pairwise, to_ego = solve_outputs(world, counts, proj_first)
    return {"world": world, "pairwise": pairwise, "to_ego": to_ego, "to_ego_f32": to_ego.astype(np.float32)}


def bits(a):
    """float32 array -> its bit patterns (NaN rows compare as patterns)"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
