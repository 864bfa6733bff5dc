"""The numpy model of the rolling voxel map (tests/_vgicp_rolling_model.py) proves itself against the models it extends and against what
include/ngicp.h states ("rolling voxel map").  No GPU.

Inserting clouds at identity must reproduce, per ijk, the merged map of the same parts in the same order to the bit: at identity
x*1 + (y*0 + (z*0 + 0)) is x and rotate_sym(I, C) is C (a product with 1.0 or 0.0 and a sum with 0.0 are exact; no covariance entry
here is a negative zero), so both models add the same doubles in the same order and divide once."""
import numpy as np
import pytest

import _vgicp_model as vm
import _vgicp_rolling_model as rm
import _vgicp_submap_model as sm


def _spd(n, seed):
    A = np.random.default_rng(seed).normal(0, 0.1, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return out


def _pose(rpy, t):
    cr, sr, cp, sp, cy, sy = np.cos(rpy[0]), np.sin(rpy[0]), np.cos(rpy[1]), np.sin(rpy[1]), np.cos(rpy[2]), np.sin(rpy[2])
    R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32)


@pytest.fixture(scope="module")
def store():
    rng = np.random.default_rng(1)
    clouds = [(rng.uniform(-3.0, 3.0, (n, 3)) + np.array(o)).astype(np.float32) for n, o in ((700, (0, 0, 0)), (601, (1.5, 0.5, 0)), (450, (-1.0, 2.0, 0.5)))]
    return clouds, [_spd(len(c), 10 + i) for i, c in enumerate(clouds)]


@pytest.mark.parametrize("res", [0.5, 1.0])
def test_inserts_at_identity_are_the_merged_map_per_voxel(store, res):
    clouds, covs = store
    r = rm.RollingVoxelMap(res)
    for p, c in zip(clouds, covs):
        r.insert(p, c, np.eye(4, dtype=np.float32))
    merged, parts = sm.merged_from_clouds(clouds, covs, [0, 1, 2], res)
    assert len(r) == len(merged)
    at = {tuple(k): v for v, k in enumerate(merged.ijk.tolist())}
    to = np.array([at[tuple(k)] for k in r.ijk.tolist()])
    assert sorted(to.tolist()) == list(range(len(merged)))  # the same voxels; only the numbering differs
    assert np.array_equal(r.count, merged.count[to])
    assert np.array_equal(r.mean, merged.mean[to]) and np.array_equal(r.cov, merged.cov[to])  # bit-equal
    # the sums themselves: the parts added in list order
    v = int(np.argmax(r.count))
    key = tuple(r.ijk[v].tolist())
    S = None
    for k in range(3):
        hit = np.flatnonzero((parts[k].ijk == np.array(key)).all(axis=1))
        if len(hit):
            S = parts[k].sum[hit[0]].copy() if S is None else S + parts[k].sum[hit[0]]
    assert np.array_equal(r.sum[v], S)
    assert r.inserts == 3 and r.stamp.max() == 3 and r.stamp.min() >= 1


def test_numbering_first_insertion_then_ascending_key(store):
    clouds, covs = store
    r = rm.RollingVoxelMap(1.0)
    n_new, n_touched = r.insert(clouds[0], covs[0], np.eye(4))
    first = r.ijk.copy()
    assert n_new == n_touched == len(first)
    keys = [(k[2], k[1], k[0]) for k in first.tolist()]
    assert keys == sorted(keys)  # one insert: ascending (iz, iy, ix), the straight map's numbering
    assert np.array_equal(first, vm.VoxelMap(clouds[0], covs[0], 1.0).ijk)
    n_new2, n_touched2 = r.insert(clouds[1], covs[1], np.eye(4))
    assert 0 < n_new2 < n_touched2  # the clouds overlap
    assert np.array_equal(r.ijk[:len(first)], first)  # numbers of existing voxels never change
    tail = [(k[2], k[1], k[0]) for k in r.ijk[len(first):].tolist()]
    assert len(tail) == n_new2 and tail == sorted(tail)
    assert (r.stamp[len(first):] == 2).all() and set(r.stamp[:len(first)].tolist()) == {1, 2}


@pytest.mark.parametrize("bad", ["far", "nan"])
def test_a_refused_insert_leaves_the_model_unchanged(store, bad):
    clouds, covs = store
    r = rm.RollingVoxelMap(0.5)
    r.insert(clouds[0], covs[0], _pose((0.1, -0.2, 0.3), (1.0, 2.0, -0.5)))
    before = r.snapshot()
    p = clouds[1].copy()
    T = np.eye(4, dtype=np.float32)
    if bad == "far":
        T[0, 3] = np.float32(0.5 * 2 ** 20)  # inside before the transform, 2^20 voxels out behind it
    else:
        p[17, 1] = np.nan
    with pytest.raises(rm.Refused):
        r.insert(p, covs[1], T)
    assert r.snapshot() == before and r.inserts == 1
    assert r.insert(clouds[1], covs[1], np.eye(4))[1] > 0 and r.inserts == 2  # the next valid insert works


def test_evict_by_distance_and_stamp(store):
    clouds, covs = store
    r = rm.RollingVoxelMap(1.0)
    for p, c in zip(clouds, covs):
        r.insert(p, c, np.eye(4))
    n = len(r)
    assert r.evict((0, 0, 0), 0.0, 0) == 0 and len(r) == n  # none: both tests off
    assert r.evict((0, 0, 0), 1e6, 1) == 0 and len(r) == n  # none: nothing that far or that old
    before = r.ijk.copy(), r.stamp.copy(), r.sum.copy()
    centre = np.array([0.25, -0.5, 0.125], np.float32)
    d2 = (((before[0] + 0.5) * 1.0 - centre.astype(np.float64)) ** 2).sum(axis=1)
    radius = float(np.sqrt(np.median(d2)))
    keep = d2 <= radius * radius
    assert r.evict(centre, radius, 0) == int((~keep).sum()) and 0 < keep.sum() < n
    assert np.array_equal(r.ijk, before[0][keep]) and np.array_equal(r.sum, before[2][keep])  # survivors' order, their state untouched
    assert np.array_equal(r.lookup((r.ijk + 0.5).astype(np.float32)), np.arange(len(r)))  # dense renumbering
    gone = before[0][~keep][0]
    assert r.lookup((gone[None] + 0.5).astype(np.float32))[0] == -1
    st = r.stamp.copy()
    assert r.evict((0, 0, 0), 0.0, 3) == int((st < 3).sum())
    assert (r.stamp == 3).all()
    assert r.evict((0, 0, 0), 0.0, 4) == len(st[st == 3]) and len(r) == 0  # all
    assert r.inserts == 3  # eviction does not touch the counter
    r.insert(clouds[0], covs[0], np.eye(4))
    assert (r.stamp == 4).all() and np.array_equal(r.ijk, vm.VoxelMap(clouds[0], covs[0], 1.0).ijk)  # numbering starts from 0 again
    r.clear()
    assert len(r) == 0 and r.inserts == 0


def test_a_reinserted_evicted_voxel_goes_to_the_end():
    rng = np.random.default_rng(3)
    A = rng.uniform(0.0, 2.0, (200, 3)).astype(np.float32)
    B = (rng.uniform(0.0, 2.0, (150, 3)) + np.array([5.0, 0.0, 0.0])).astype(np.float32)  # shares no voxel with A
    cA, cB = _spd(len(A), 1), _spd(len(B), 2)
    r = rm.RollingVoxelMap(1.0)
    r.insert(A, cA, np.eye(4))
    old = r.ijk.copy()
    r.insert(B, cB, np.eye(4))
    assert np.array_equal(r.ijk[:len(old)], old)
    assert r.evict((0, 0, 0), 0.0, 2) == len(old)  # A's voxels are older than insert 2
    n = len(r)
    assert n > 0 and r.lookup(A).max() == -1
    assert np.array_equal(r.lookup((r.ijk + 0.5).astype(np.float32)), np.arange(n))
    n_new, n_touched = r.insert(A, cA, np.eye(4))
    assert n_new == n_touched == len(old)
    assert np.array_equal(r.ijk[n:], old) and r.lookup(A).min() >= n  # new numbers at the end, not the old ones
    assert (r.stamp[n:] == 3).all() and (r.stamp[:n] == 2).all()


def test_a_rotated_inserts_covariance_sum_is_the_rotation_of_the_sum(store):
    clouds, covs = store
    T = _pose((0.3, -0.7, 1.1), (0.4, -0.2, 0.9))
    r = rm.RollingVoxelMap(1.0)
    r.insert(clouds[0], covs[0], T)
    q = rm.transform_pcl_f32(T, clouds[0])
    straight = vm.VoxelMap(q, covs[0], 1.0)  # the same voxels (one insert: the same numbering), covariances not rotated
    assert np.array_equal(r.ijk, straight.ijk) and np.array_equal(r.count, straight.count)
    assert np.array_equal(r.mean, straight.mean)
    R = T[:3, :3].astype(np.float64)
    C = vm.cov3(covs[0])
    for v in (0, len(r) // 2, len(r) - 1, int(np.argmax(r.count))):
        c = np.zeros((3, 3))
        for j in straight.members[v]:
            c = c + C[j]
        assert np.array_equal(r.covsum[v], rm.rotate_sym(R, c))  # one rotation, of the sum
        per_point = sum(R @ C[j] @ R.T for j in straight.members[v])
        assert np.allclose(r.covsum[v], per_point, rtol=1e-12, atol=0)  # and, to rounding, the sum of the rotations
        assert np.array_equal(r.covsum[v], r.covsum[v].T)
    assert np.array_equal(rm.rotate_sym(np.eye(3), C[5]), C[5])
