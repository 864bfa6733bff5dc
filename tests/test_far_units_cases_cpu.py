"""The inputs of tests/test_gpu_far_units.py do what its tests claim (no GPU): tests/_far_units_cases.py's numpy restatement of the
engine's grid says that every query of the sandwich lies beyond ring 1 of its nearest target point, that its cold pass queues more than
kUnitCap far units in some batch, and that the ties are exact ties across different rows."""
import numpy as np
import pytest

import _far_units_cases as fc
import _index_history_cases as ic
from direct_lidar_odometry_amd import clouds


@pytest.fixture(scope="module")
def sandwich():
    src, tgt = fc.sandwich()
    q = clouds.transform_points(fc.GUESS, src).astype(np.float32)
    return src, tgt, q


def test_sandwich_grid_and_distances(sandwich):
    src, tgt, q = sandwich
    assert src.dtype == tgt.dtype == np.float32 and src.shape == (1500, 3) and tgt.shape == (9601, 3)
    dims, h = ic.grid_of(tgt, fc.VOXEL)
    assert h == np.float32(fc.VOXEL) and dims == [20, 20, 14]
    d = np.sqrt(((q[:, None, :].astype(np.float64) - tgt[None, :, :]) ** 2).sum(2).min(1))
    print(f"nearest target point: {d.min() / fc.VOXEL:.2f} .. {d.max() / fc.VOXEL:.2f} voxels")
    assert d.min() > 1.5 * fc.VOXEL and d.max() < 3.5 * fc.VOXEL and d.max() < fc.GATE  # beyond ring 1, inside the gate
    # ring 1 of every query's cell is empty: the search cannot end there
    tc = {tuple(c) for c in ic.cell_coords(tgt, tgt.min(0), h, dims)[:, 1:]}
    qc = ic.cell_coords(q, tgt.min(0), h, dims)[:, 1:]
    assert not any((y + dy, z + dz) in tc for y, z in qc for dy in (-1, 0, 1) for dz in (-1, 0, 1))
    # the gate spans at least three rings, and no more than the stage lists
    assert 3 <= int(np.ceil(fc.GATE / fc.VOXEL)) <= 6


def test_sandwich_cold_pass_needs_more_than_one_round(sandwich):
    """Every query has at least 33 non-empty rows beyond ring 1 within the gate (the cold pass has no other bound), so a batch that
    queues kUnitCap units or fewer holds at most 8 queries - and 1500 queries in 9 tiles cannot all sit in such batches."""
    src, tgt, q = sandwich
    n_all, n_far = fc.rows_within_reach(q, tgt, fc.VOXEL, fc.GATE)
    tiles = fc.occupied_tiles(src, fc.VOXEL)
    print(f"rows within the gate per query: {n_all.min()} .. {n_all.max()}, beyond ring 1: {n_far.min()} .. {n_far.max()}; occupied tiles {tiles}")
    assert n_far.min() >= 33 and tiles <= 9
    assert fc.BATCH * int(n_far.min()) > fc.UNIT_CAP  # a full batch exceeds the cap several times over
    assert fc.some_batch_exceeds_cap(len(src), tiles, int(n_far.min()))
    assert not fc.some_batch_exceeds_cap(len(src), tiles, 1)  # (the argument can fail)
    # the region of a batch (a tile of 4 x 4 cells, a cell more for the pose, 5 rings around it) fits the row tables: 256 rows of 20 cells
    rings = int(np.ceil(fc.GATE / fc.VOXEL))
    dims, _ = ic.grid_of(tgt, fc.VOXEL)
    assert (5 + 2 * rings) * min(dims[2], 2 + 2 * rings) <= 256 and 5 + 2 * rings <= ic.STAGE_XS


def test_short_batch_sources_are_single_patches(sandwich):
    src, _, _ = sandwich
    for n in (33, 45):
        part = src[np.argsort(np.abs(src[:, :2] - src[0, :2]).max(1))[:n]]
        assert len(part) == n and n % fc.BATCH != 0 and fc.occupied_tiles(part, fc.VOXEL) <= 4


def test_ties_are_exact_and_across_rows():
    src, tgt, winners = fc.ties()
    assert src.dtype == tgt.dtype == np.float32 and len(src) == 64
    d = [src[:, None, r] - tgt[None, :, r] for r in range(3)]  # float32, the identity pose leaves the queries as they are
    D = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    order = np.argsort(D, axis=1, kind="stable")
    best = np.take_along_axis(D, order[:, :3], 1)
    assert np.all(best[:, 0] == np.float32(0.0625)) and np.all(best[:, 1] == np.float32(0.0625)) and np.all(best[:, 2] > np.float32(0.0625))
    dims, h = ic.grid_of(tgt, fc.VOXEL)
    mn = tgt.min(0)
    tc, qc = ic.cell_coords(tgt, mn, h, dims), ic.cell_coords(src, mn, h, dims)
    for i in range(len(src)):
        a, b = sorted(order[i, :2])
        assert b == winners[i] and a == i  # the pair of query i: the upper point first in the cloud, the lower one second
        ra, rb = tc[a, 1:], tc[b, 1:]
        assert tuple(ra) != tuple(rb)  # different rows
        assert all(max(abs(r[0] - qc[i, 1]), abs(r[1] - qc[i, 2])) >= 2 for r in (ra, rb))  # both beyond ring 1
        assert (rb[1], rb[0]) < (ra[1], ra[0])  # the winner's row comes first in the cell-sorted target (z, then y)
