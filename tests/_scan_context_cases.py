"""Fixtures shared by the scan context tests: scans along a drive through clouds.make_scene(), yawed revisits, and the margins the GPU
tests rely on (asserted on the MODEL, before the engine is looked at)."""
import functools

import numpy as np

import _scan_context_model as scm
from direct_lidar_odometry_amd import clouds

COLS = 188           # 16 x 188 = 3 008 points per scan
MARGIN = 1e-6        # what two model values must differ by before the engine is asked to tell them apart
REVISIT_YAW_DEG = 37.0
REVISIT_MOVE = (0.32, 0.24, 0.0)  # 0.4 m


@functools.lru_cache(maxsize=None)
def scene():
    return clouds.make_scene()


def drive_pose(i, n):
    """place i of n along an S-shaped drive through the room, heading along the path"""
    u = i / max(n - 1, 1)
    x, y = -15.0 + 30.0 * u, 8.0 * np.sin(2.0 * np.pi * u)
    heading = np.degrees(np.arctan2(8.0 * 2.0 * np.pi * np.cos(2.0 * np.pi * u), 30.0))
    return clouds.make_pose((x, y, 0.0), (0.0, 0.0, heading))


@functools.lru_cache(maxsize=None)
def drive_scans(n, seed=500):
    return tuple(clouds.vlp16(scene(), drive_pose(i, n), noise_seed=seed + i, cols=COLS) for i in range(n))


def revisit(i, n, yaw_deg=REVISIT_YAW_DEG, move=REVISIT_MOVE, seed=900):
    """-> (scan, T): a scan taken at place i with the sensor yawed by yaw_deg and moved by `move` (in the place's frame), and the 4x4
    that carries it into the frame of place i's scan"""
    T = clouds.make_pose(move, (0.0, 0.0, yaw_deg))
    return clouds.vlp16(scene(), drive_pose(i, n) @ T, noise_seed=seed + i, cols=COLS), T


@functools.lru_cache(maxsize=None)
def default_tables():
    return scm.tables(*scm.DEFAULTS[:3])


def margins(Q, database):
    """-> (smallest gap between a candidate's two smallest d_k, smallest gap between neighbouring ranked distances) in the model"""
    shift_gap, dist = np.inf, []
    for C in database:
        d = np.sort(scm.shift_distances(Q, C))
        shift_gap = min(shift_gap, d[1] - d[0])
        dist.append(d[0])
    rank_gap = np.diff(np.sort(dist)).min() if len(dist) > 1 else np.inf
    return shift_gap, rank_gap
