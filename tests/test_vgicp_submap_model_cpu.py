"""The numpy model of the merged voxel map (tests/_vgicp_submap_model.py) against the model of the straight one
(_vgicp_model.VoxelMap of the concatenation): what include/ngicp.h states as consequences of the definition.  No GPU.

The bound on a mean or covariance entry.  Such an entry is (x_1 + ... + x_n) / n with n = n_v, the x_j being the coordinates (or the
covariance entries) of the voxel's points.  A recursive IEEE double sum of n terms in any order is off the exact sum by at most
(n - 1) u sum|x_j| to first order, u = 2^-53; two orders are therefore at most 2 (n - 1) u sum|x_j| apart, after the division by n
at most 2 u sum|x_j| (n - 1) / n, and each division adds at most u |entry| <= u sum|x_j| / n: together below 2 u sum|x_j|.  The
issue's bound doubles that for the higher-order terms: 4 * 2^-53 * sum|x_j|.  Derived, not measured."""
import numpy as np
import pytest

import _vgicp_model as vm
import _vgicp_submap_model as sm

U = 2.0 ** -53


def _spd(n, seed):
    A = np.random.default_rng(seed).normal(0, 0.1, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return out


@pytest.fixture(scope="module")
def store():
    """Three overlapping keyframes (dense: voxels of a few dozen points) and their covariances."""
    rng = np.random.default_rng(1)
    clouds = [(rng.uniform(-3.0, 3.0, (n, 3)) + np.array(o)).astype(np.float32) for n, o in ((1500, (0, 0, 0)), (1201, (1.5, 0.5, 0)), (900, (-1.0, 2.0, 0.5)))]
    covs = [_spd(len(c), 10 + i) for i, c in enumerate(clouds)]
    return clouds, covs


def _straight(store, ids, res):
    clouds, covs = store
    return vm.VoxelMap(np.concatenate([clouds[k] for k in ids]), np.concatenate([covs[k] for k in ids]), res), np.concatenate([clouds[k] for k in ids]), np.concatenate([covs[k] for k in ids])


def _within_bound(merged, straight, pts, covs, label):
    p64, C = pts.astype(np.float64), vm.cov3(covs)
    worst = 0.0
    for v, idx in enumerate(straight.members):
        bm = 4 * U * np.abs(p64[idx]).sum(axis=0)
        bc = 4 * U * np.abs(C[idx]).sum(axis=0)
        dm, dc = np.abs(merged.mean[v] - straight.mean[v]), np.abs(merged.cov[v] - straight.cov[v])
        assert (dm <= bm).all() and (dc <= bc).all(), f"{label}: voxel {v} ({len(idx)} points) is off by {dm.max():.2e} / {dc.max():.2e}"
        worst = max(worst, (dm / bm).max(), (dc / np.maximum(bc, 1e-300)).max())
    print(f"{label}: {len(straight)} voxels, largest count {straight.count.max()}, largest difference {worst:.3f} of its bound")


@pytest.mark.parametrize("ids", [[0, 1, 2], [0, 2], [2, 0], [1], [0, 0], [2, 1, 0, 1]])
@pytest.mark.parametrize("res", [0.5, 1.0, 4.0])
def test_the_merged_map_has_the_voxels_and_counts_of_the_straight_one(store, ids, res):
    clouds, covs = store
    merged, _ = sm.merged_from_clouds(clouds, covs, ids, res)
    straight, pts, cc = _straight(store, ids, res)
    assert np.array_equal(merged.ijk, straight.ijk) and np.array_equal(merged.count, straight.count)
    assert merged.count.sum() == len(pts)
    _within_bound(merged, straight, pts, cc, f"{ids} at {res}")
    q = np.r_[pts[::7], np.array([[500, 500, 500], [3e6, 0, 0], [np.nan, 0, 0]], np.float32)]
    assert np.array_equal(merged.lookup(q), straight.lookup(q))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_keyframe_gives_the_straight_map_bit_for_bit(store, k):
    clouds, covs = store
    merged, parts = sm.merged_from_clouds(clouds, covs, [k], 1.0)
    straight = vm.VoxelMap(clouds[k], covs[k], 1.0)
    assert np.array_equal(merged.ijk, straight.ijk) and np.array_equal(merged.count, straight.count)
    assert np.array_equal(merged.mean, straight.mean) and np.array_equal(merged.cov, straight.cov)
    # the part itself: the straight map's sums before the division
    p = parts[k]
    assert np.array_equal(p.ijk, straight.ijk) and np.array_equal(p.count, straight.count)
    assert np.array_equal(p.sum / p.count[:, None], straight.mean) and np.array_equal(p.covsum / p.count[:, None, None], straight.cov)


def test_several_keyframes_do_change_the_rounding(store):
    """The merged map is another definition, not another route to the same bits: on this data some entry differs."""
    clouds, covs = store
    merged, _ = sm.merged_from_clouds(clouds, covs, [0, 1, 2], 1.0)
    straight, _, _ = _straight(store, [0, 1, 2], 1.0)
    assert not (np.array_equal(merged.mean, straight.mean) and np.array_equal(merged.cov, straight.cov))


def test_an_id_listed_twice_doubles_the_counts(store):
    clouds, covs = store
    once, _ = sm.merged_from_clouds(clouds, covs, [0, 1], 1.0)
    twice, _ = sm.merged_from_clouds(clouds, covs, [0, 1, 0, 1], 1.0)
    assert np.array_equal(once.ijk, twice.ijk) and np.array_equal(2 * once.count, twice.count)
    one, _ = sm.merged_from_clouds(clouds, covs, [0], 1.0)
    two, _ = sm.merged_from_clouds(clouds, covs, [0, 0], 1.0)
    assert np.array_equal(2 * one.count, two.count)
    assert np.array_equal(one.mean, two.mean) and np.array_equal(one.cov, two.cov)  # (S + S) / 2n = S / n exactly: doubling is exact


def test_the_order_of_the_ids_changes_rounding_only(store):
    clouds, covs = store
    a, _ = sm.merged_from_clouds(clouds, covs, [0, 1], 1.0)
    b, _ = sm.merged_from_clouds(clouds, covs, [1, 0], 1.0)
    assert np.array_equal(a.ijk, b.ijk) and np.array_equal(a.count, b.count)
    straight, pts, cc = _straight(store, [0, 1], 1.0)
    _within_bound(a, straight, pts, cc, "[0, 1]")
    _within_bound(b, straight, pts, cc, "[1, 0]")
    # two parts: a + b == b + a in IEEE arithmetic, so here the two orders even agree to the bit
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.cov, b.cov)


def test_a_point_beyond_the_range_refuses_the_part():
    pts = np.array([[0.5, 0.5, 0.5], [262144.0, 0, 0]], np.float32)
    with pytest.raises(ValueError):
        sm.VoxelPart(pts, _spd(2, 3), 0.25)
    assert len(sm.VoxelPart(pts, _spd(2, 3), 1.0)) == 2
    pts[1, 0] = np.nan
    with pytest.raises(ValueError):
        sm.VoxelPart(pts, _spd(2, 3), 1.0)
