"""Inputs of tests/test_gpu_far_units.py (the listed-row, "far", units of ngicp_pass_group.inc), with a numpy restatement of what the far
section queues for them; tests/test_far_units_cases_cpu.py shows on the CPU that the inputs do what the GPU tests claim.  Not collected
by pytest (no test_ prefix).

sandwich   two dense slabs (z in [-0.4, 0] and [0.6, 1.0], 2 m x 2 m) and a source sheet held between them at z = 0.3 +- 0.03: every
           query's nearest target point is 2.7 .. 3.3 voxels away at the pinned 0.1 m voxel, on either side (so the alignment leaves the
           sheet where it is: the queries stay far in every pass).  With the 0.5 m gate five rings cover the gate; in the cold first pass
           (no bound but the gate) every query has some thirty listed rows within reach, so every batch of ten queries or more queues
           more than kUnitCap units: more than one round.
ties       queries on a dyadic lattice (1/16 m apart in x) under the identity pose, each with two target points at bit-equal float32 distance in two different
           listed rows (y - 0.25 / y + 0.25, or z - 0.25 / z + 0.25): rings 2-3 at the 0.1 m voxel.
"""
import numpy as np

import _index_history_cases as ic
from direct_lidar_odometry_amd import clouds

UNIT_CAP = 288   # kUnitCap (ngicp_search.h)
TILE_SHIFT = 2   # query batches never leave a tile of 2^2 cells per axis of the source's grid (ngicp_api.hip)
BATCH = 32       # kBatchQueries
VOXEL = 0.1
GATE = 0.5
ISO_COV = ic.ISO_COV
SETTINGS = dict(setMaximumIterations=5, setTransformationEpsilon=1e-9, setRotationEpsilon=1e-9)  # at most six passes
GUESS = clouds.make_pose((0.02, -0.015, 0.0), (0.0, 0.0, 0.5))


def sandwich(n_src=1500):
    """(source, target): see the module docstring.  The first target point is the box corner (-0.4 m below the lower slab's top)."""
    rng = np.random.default_rng(201)
    lo = np.c_[rng.uniform(0.0, 2.0, (4800, 2)), rng.uniform(-0.4, 0.0, 4800)]
    hi = np.c_[rng.uniform(0.0, 2.0, (4800, 2)), rng.uniform(0.6, 1.0, 4800)]
    tgt = np.r_[[[0.0, 0.0, -0.4]], lo, hi].astype(np.float32)
    src = np.c_[rng.uniform(0.4, 1.6, (n_src, 2)), rng.uniform(0.27, 0.33, n_src)].astype(np.float32)
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt)


def rows_within_reach(q, tgt, voxel, reach):
    """Per query point of q (already under the pose): the number of non-empty (y, z) grid rows of the target whose cell square lies
    within `reach` of the query in (y, z) - row_gap_sq without the grid's slack, which only lets more rows through - and how many of
    them lie beyond ring 1 of the query's cell.  Every one of them that the batch's region lists becomes a unit in the cold pass."""
    dims, h = ic.grid_of(tgt, voxel)
    mn = tgt.min(0).astype(np.float32)
    tc = ic.cell_coords(tgt, mn, h, dims)
    occupied = np.zeros((dims[1], dims[2]), bool)
    occupied[tc[:, 1], tc[:, 2]] = True
    qc = ic.cell_coords(q, mn, h, dims)
    ys = mn[1] + np.arange(dims[1] + 1) * float(h)
    zs = mn[2] + np.arange(dims[2] + 1) * float(h)
    n_all, n_far = np.zeros(len(q), int), np.zeros(len(q), int)
    for i, (p, c) in enumerate(zip(q, qc)):
        gy = np.maximum(np.maximum(ys[:-1] - p[1], p[1] - ys[1:]), 0.0)
        gz = np.maximum(np.maximum(zs[:-1] - p[2], p[2] - zs[1:]), 0.0)
        near = (gy[:, None] ** 2 + gz[None, :] ** 2 <= reach ** 2) & occupied
        ring = np.maximum(np.abs(np.arange(dims[1]) - c[1])[:, None], np.abs(np.arange(dims[2]) - c[2])[None, :])
        n_all[i], n_far[i] = near.sum(), (near & (ring > 1)).sum()
    return n_all, n_far


def occupied_tiles(src, voxel):
    """Tiles of the source's own grid that hold a source point: a query batch never leaves one."""
    dims, h = ic.grid_of(src, voxel)
    c = ic.cell_coords(src, src.min(0).astype(np.float32), h, dims) >> TILE_SHIFT
    return len(np.unique(c, axis=0))


def some_batch_exceeds_cap(n, tiles, rows_min):
    """True if n queries in `tiles` tiles, each with at least rows_min units to queue, cannot all sit in batches that queue kUnitCap units
    or fewer: a batch that fits holds at most k = kUnitCap // rows_min queries, and there are at most tiles + n / 32 batches."""
    k = UNIT_CAP // rows_min
    return k < BATCH and n > k * (tiles + n / BATCH)


def ties():
    """(source, target, winners): 64 queries at (i / 16, 1, 1); the first 32 with target points at y = 0.75 and y = 1.25, the others at
    z = 0.75 and z = 1.25, all at the query's x: both at squared distance 0.0625 exactly.  The point in the LOWER row (smaller z, then smaller y:
    the cell-sorted order) has the HIGHER index in the target as given.  winners[i]: the index that must win."""
    n = 64
    x = np.arange(n, dtype=np.float32) / np.float32(16.0)  # (exact in float32)
    src = np.c_[x, np.ones(n, np.float32), np.ones(n, np.float32)].astype(np.float32)
    hi, lo = src.copy(), src.copy()
    hi[:32, 1] += 0.25; lo[:32, 1] -= 0.25
    hi[32:, 2] += 0.25; lo[32:, 2] -= 0.25
    corners = np.array([[0.0, 0.75, 0.75], [(n - 1.0) / 16.0, 1.25, 1.25]], np.float32)  # the grid's box: both axes split into rows
    tgt = np.ascontiguousarray(np.r_[hi, lo, corners].astype(np.float32))
    return np.ascontiguousarray(src), tgt, n + np.arange(n)
