"""Fixtures shared by the pose search tests: the end-to-end scene on the scan-context drive (tests/_scan_context_cases.py) - a rolling
map of the 12 drive scans carried into the frame of place 5, a revisit of place 5 yawed by 37 degrees and moved by a few metres - and
the model's answer on it, computed once per process."""
import functools

import numpy as np

import _pose_search_model as psm
import _scan_context_cases as cs
from _vgicp_model import voxel_of
from _vgicp_rolling_model import transform_pcl_f32

F = np.float32
RES = 0.5
PLACE, N_PLACES = 5, 12
MOVES = ((2.3, -1.7, 0.0), (4.1, 3.3, 0.0))
EXTENT = (12, 12, 1)
N_YAWS, YAW_STEP = 72, np.radians(5.0)


@functools.lru_cache(maxsize=None)
def insert_poses():
    """the float32 pose that carries scan i of the drive into the frame of place 5"""
    inv = np.linalg.inv(cs.drive_pose(PLACE, N_PLACES))
    return tuple((inv @ cs.drive_pose(i, N_PLACES)).astype(F) for i in range(N_PLACES))


@functools.lru_cache(maxsize=None)
def map_cells():
    """the cells of the rolling map after the 12 inserts (an insert moves a point as pcl::transformPointCloud does)"""
    got = [voxel_of(transform_pcl_f32(T, s), RES) for T, s in zip(insert_poses(), cs.drive_scans(N_PLACES))]
    return np.unique(np.concatenate(got), axis=0)


@functools.lru_cache(maxsize=None)
def lattice():
    return psm.yaw_lattice(np.eye(4), N_YAWS, YAW_STEP)


@functools.lru_cache(maxsize=None)
def query(move):
    """-> (scan, T_true): the revisit of place 5 and the pose that carries it into place 5's frame"""
    return cs.revisit(PLACE, N_PLACES, move=move)


@functools.lru_cache(maxsize=None)
def model_volume(move):
    return psm.score_volume(lattice(), query(move)[0], map_cells(), RES, EXTENT)


def model_top(move, top_k=8):
    return psm.ranking(model_volume(move), top_k)
