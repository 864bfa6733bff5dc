"""The clouds, covariances, poses and record sets that test_vgicp_rollmap_model_cpu.py (the model's own properties) and
test_gpu_vgicp_rollmap.py (the engine against the model) share.   *** TEST INFRASTRUCTURE ONLY ***   Not collected by pytest.

The maps are built from VLP-16 scans of 188 columns (3008 points), as tests/test_gpu_vgicp_rolling.py builds them, with covariances
that are set, not computed: the CPU test then works on exactly the numbers the GPU test feeds the engine."""
from __future__ import annotations

import functools

import numpy as np

from _vgicp_rollmap_model import RecordVoxelMap
from direct_lidar_odometry_amd import clouds

RES = 1.0
I4 = np.eye(4, dtype=np.float32)
# a pose that makes records merge: 0.3 rad about z (and a little about x, y), 1.3 m
T_MERGE = clouds.make_pose((1.2, -0.4, 0.3), (2.0, -3.0, np.degrees(0.3))).astype(np.float32)
assert abs(np.linalg.norm(T_MERGE[:3, 3]) - 1.3) < 1e-6
# a pose whose float image is the identity: the diagonal differs from 1 by less than half a float ulp
T_NEARLY_I = np.eye(4) + np.diag([1e-9, -2e-9, 3e-9, 0.0])
assert np.array_equal(T_NEARLY_I.astype(np.float32), I4) and not np.array_equal(T_NEARLY_I, np.eye(4))


def spd(n, seed):
    """n random symmetric positive definite 3x3 matrices as (n, 4, 4) covariances (tests/test_gpu_vgicp_rolling.py)."""
    A = np.random.default_rng(seed).normal(0, 0.1, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return out


@functools.lru_cache(maxsize=None)
def drive():
    """Six scans along a path with their float poses and covariances: 0..2 build the map, 3 is aligned against it, 4 is the further
    insert, 5 builds a second map."""
    sc = clouds.make_scene()
    gts = [clouds.make_pose((0.4 * i, 0.1 * i, 0.0), (0.0, 0.0, 1.5 * i)) for i in range(6)]
    scans = [clouds.vlp16(sc, gts[i], 200 + i, cols=188) for i in range(6)]
    assert all(len(s) == 3008 for s in scans)
    return dict(scans=scans, covs=[spd(len(s), 700 + i) for i, s in enumerate(scans)], poses=[g.astype(np.float32) for g in gts], gts=gts)


EVICT = dict(centre=(0.4, 0.1, 0.0), max_dist=20.3, min_stamp=0)  # of the built map: by distance, so that stamps 1, 2 and 3 all survive


def built_model(res=RES, n_scans=3, evict=True) -> RecordVoxelMap:
    """A fresh model of the map every test starts from: scans 0..n_scans-1 at their poses, then one eviction."""
    d = drive()
    m = RecordVoxelMap(res)
    for s, c, T in zip(d["scans"][:n_scans], d["covs"], d["poses"]):
        m.insert(s, c, T)
    if evict:
        assert m.evict(**EVICT) > 0
    return m


@functools.lru_cache(maxsize=None)
def built_records(res=RES):
    """(ijk, S, C, count, stamp, inserts) of built_model(res): read-only, shared"""
    m = built_model(res)
    out = (*m.records(), m.inserts)
    for a in out[:5]:
        a.setflags(write=False)
    return out


def one_voxel_records(n=3000, seed=11):
    """n records whose means lie within a centimetre of one another, well inside one voxel: one long segment"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 40, n)
    mean = np.array([5.5, -3.5, 0.5]) + rng.uniform(-0.005, 0.005, (n, 3))
    return mean * cnt[:, None], spd(n, seed + 1)[:, :3, :3] * cnt[:, None, None], cnt
