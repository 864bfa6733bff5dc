"""Clearing the rolling voxel map along a scan's rays (include/ngicp.h "rolling voxel map: clearing along rays", csrc/ngicp_voxel_ray.h)
against the numpy model of that definition (tests/_vgicp_ray_model.py): miss, hit, the three totals, n_removed and - after a removal -
every array of rollingVoxelMap(), np.array_equal throughout.  Maps are made with setRollingVoxelMap, so means sit where a case needs them."""
import numpy as np
import pytest

import _vgicp_ray_drive as drive
import _vgicp_ray_model as ray
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -2, -3
I4 = np.eye(4, dtype=np.float32)
T_RIGID = clouds.make_pose((1.3, -0.7, 0.4), (10.0, -20.0, 30.0)).astype(np.float32)
TOTALS = ("steps", "occupied", "misses", "n_removed")


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _spd(n, seed):
    A = np.random.default_rng(seed).normal(0, 0.1, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return out


def _cube(n, half, seed, offset=(0.0, 0.0, 0.0)):
    return (np.random.default_rng(seed).uniform(-half, half, (n, 3)) + np.asarray(offset)).astype(np.float32)


def _lattice_planes(res):
    """Points exactly on lattice planes, negative ones included, some twice; and points just below a plane (tests/test_gpu_vgicp_rolling.py)."""
    k = np.arange(-6, 7, dtype=np.float32) * np.float32(res)
    p = np.stack(np.meshgrid(k, k[::3], k[::4], indexing="ij"), -1).reshape(-1, 3)
    below = np.nextafter(p[::5], np.float32(-np.inf))
    return np.ascontiguousarray(np.r_[p, p[::7], below, np.array([[-0.0, 0.0, -0.0]], np.float32)])


def _raises(ng, code, fn, *a, **kw):
    with pytest.raises(ng.NgicpError) as e:
        fn(*a, **kw)
    assert e.value.code == code, f"{e.value}"


def _block(lo, hi):
    k = np.arange(lo, hi)
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)


class Ray:
    """A handle with the rolling setting on and a producer that feeds it."""

    def __init__(self, ng, res=1.0):
        self.ng, self.res = ng, res
        self.prod, self.g = ng.NanoGICP(), ng.NanoGICP()
        self.g.setVoxelResolution(res)
        self.g.setVoxelRolling(True)

    def set_map(self, ijk, mean=None, stamp=None, inserts=None):
        """one point per voxel, so the record's mean is `mean` itself (default: the cell's centre)"""
        ijk = np.asarray(ijk, np.int32).reshape(-1, 3)
        mean = (ijk + 0.5) * self.res if mean is None else np.asarray(mean, np.float64)
        stamp = np.ones(len(ijk), np.int64) if stamp is None else np.asarray(stamp, np.int64)
        self.g.setRollingVoxelMap(ijk, mean, np.tile(0.01 * np.eye(3), (len(ijk), 1, 1)), np.ones(len(ijk), np.int32), stamp,
                                  int(stamp.max(initial=0)) if inserts is None else inserts)

    def source(self, pts):
        self.prod.setInputSource(np.ascontiguousarray(pts, np.float32), identity=0)  # (0: always uploaded, whatever the array's address)

    def model(self, pts, T=I4, origin=None, **opt):
        ijk, S, _, cnt, st = self.g.rollingVoxelMap()
        return ray.ray_clear(ijk, S / cnt.astype(np.float64)[:, None], st, self.res, pts, T, origin, **opt)

    def clear(self, pts, T=I4, origin=None, label="", **opt):
        """the engine's call against the model's on the engine's present state -> (the engine's result, the model's)"""
        before, stats0 = self.g.rollingVoxelMap(), self.g.voxelRollingStats()
        want = self.model(pts, T, origin, **opt)
        self.source(pts)
        got = self.g.clearVoxelMapAlongRays(self.prod, T, origin, **opt)
        miss, hit = self.g.voxelMapRayCounts()
        assert miss.dtype == hit.dtype == np.uint32
        assert np.array_equal(miss, want["miss"]), f"{label}: miss"
        assert np.array_equal(hit, want["hit"]), f"{label}: hit"
        assert [got[k] for k in TOTALS] == [want[k] for k in TOTALS], f"{label}: the engine {got}, the model {[want[k] for k in TOTALS]}"
        assert got["kernel_ms"] >= 0.0
        after, stats1 = self.g.rollingVoxelMap(), self.g.voxelRollingStats()
        for a, b in zip(after, before):
            assert a.dtype == b.dtype and np.array_equal(a, b[want["keep"]]), f"{label}: the map behind the call"
        assert stats1["inserts"] == stats0["inserts"] and stats1["n_vox"] == int(want["keep"].sum()), label
        return got, want

    def close(self):
        self.prod.close(); self.g.close()


@pytest.fixture(scope="module")
def block(ng):
    """8 x 8 x 8 occupied cells [-4, 4)^3 at 1 m: every step inside is a probe hit"""
    r = Ray(ng, 1.0)
    r.set_map(_block(-4, 4))
    yield r
    r.close()


O = np.array([0.5, 0.5, 0.5], np.float32)
WALK_EDGES = {
    "inside one cell (N = 0)": (O, [[0.7, 0.2, 0.9]]),
    "N = 1": (O, [[1.5, 0.5, 0.5]]),
    "N = 3 <= near + back": (O, [[2.5, 1.5, 0.5], [1.5, 1.5, 1.5]]),
    "axis-aligned, both directions": (O, [[3.5, 0.5, 0.5], [-3.5, 0.5, 0.5], [0.5, 3.5, 0.5], [0.5, -3.5, 0.5], [0.5, 0.5, 3.5], [0.5, 0.5, -3.5],
                                          [6.5, 0.5, 0.5], [0.5, -6.5, 0.5]]),
    "negative coordinates": (np.array([-3.3, -2.7, -1.1], np.float32), _cube(40, 3.0, 1, (-3.5, -3.5, -3.5))),
    "lattice planes, one ulp below, -0.0": (np.array([0.3, 0.2, 0.1], np.float32), _lattice_planes(1.0)),
    "an origin on a lattice corner": (np.array([-0.0, 1.0, -2.0], np.float32), _lattice_planes(1.0)[::3]),
    "corner diagonals (ties of two and three)": (O, O + np.array([[5, 5, 5], [-5, -5, -5], [4, 4, 0], [0, -4, -4], [4, 0, 4], [-3, 3, 3], [3, 3, -3], [6, 3, 3]], np.float32)),
}


@pytest.mark.parametrize("case", list(WALK_EDGES))
def test_walk_edges(block, case):
    o, q = WALK_EDGES[case]
    q = np.asarray(q, np.float32)
    for radius in (0.0, 0.25):
        got, want = block.clear(q, I4, o, case, dry_run=1, back_cells=0 if "diagonal" in case or "axis" in case else 2, radius_cells=radius)
    print(f"{case}: {len(q)} rays, {want['steps']} counted steps, {want['occupied']} occupied, {want['misses']} misses, {int(want['hit'].sum())} hits")
    if "N = 0" in case or "N = 1" in case or "N = 3" in case:
        assert want["steps"] == 0 and want["hit"].sum() == len(q)
    else:
        assert want["occupied"] > 0 and want["misses"] > 0


@pytest.mark.parametrize("opt", [dict(near_cells=3), dict(back_cells=0), dict(max_steps=1), dict(max_steps=5), dict(near_cells=3, back_cells=0, max_steps=5)],
                         ids=lambda o: " ".join(f"{k}={v}" for k, v in o.items()))
def test_option_edges(block, opt):
    q = np.r_[_cube(60, 3.9, 2), _cube(20, 12.0, 3)]  # rays that end inside the block and long ones that leave it
    base = block.model(q, I4, O, radius_cells=0.0)
    got, want = block.clear(q, I4, O, str(opt), dry_run=1, radius_cells=0.0, **opt)
    assert want["steps"] != base["steps"] and want["misses"] > 0
    if "max_steps" in opt:
        assert want["steps"] <= opt["max_steps"] * len(q)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1030])
def test_ray_counts_around_the_wave_and_the_block(block, n):
    q = _cube(n, 6.0, 10 + n)
    got, want = block.clear(q, T_RIGID, None, f"{n} rays", dry_run=1)
    got0, want0 = block.clear(q, T_RIGID, None, f"{n} rays, the cell test alone", dry_run=1, radius_cells=0.0)
    assert want0["steps"] == want["steps"] and want0["misses"] == want0["occupied"] >= want["misses"]


def test_every_step_inside_the_block_is_a_probe_hit(block):
    q = _cube(300, 3.9, 4)
    got, want = block.clear(q, I4, O, "inside the block", dry_run=1, back_cells=0)
    assert want["steps"] == want["occupied"] > 300


def test_one_long_ray_among_short_ones_in_a_wave(ng):
    r = Ray(ng, 1.0)
    cells = np.r_[np.array([[i, i, i] for i in range(1, 200, 3)]), [[1, 0, 0], [0, 1, 0]]]
    r.set_map(cells)
    q = np.tile(np.array([[1.5, 0.5, 0.5]], np.float32), (64, 1))
    q[37] = (200.5, 200.5, 200.5)
    got, want = r.clear(q, I4, O, "600 steps among one-step rays", dry_run=1, back_cells=0)
    assert want["steps"] == 599 and want["occupied"] > 60 and want["hit"][len(cells) - 2] == 63
    got, want = r.clear(q, I4, O, "the long ray removes its voxels", back_cells=0, min_miss=1)
    assert got["n_removed"] == want["misses"] == 67 and want["occupied"] == 68  # ((1, 0, 0) is entered off its mean, and 63 rays end in it)
    r.close()


def test_4096_rays_through_one_voxel(ng):
    r = Ray(ng, 1.0)
    r.set_map([[3, 0, 0], [20, 20, 20]])
    q = np.c_[np.full(4096, 9.5), 0.5 + np.random.default_rng(5).uniform(-0.4, 0.4, 4096), np.full(4096, 0.5)].astype(np.float32)
    got, want = r.clear(q, I4, O, "4096 rays, min_miss 4097", min_miss=4097)
    assert want["miss"].tolist() == [4096, 0] and got["n_removed"] == 0
    got, want = r.clear(q, I4, O, "4096 rays, min_miss 4096", min_miss=4096)
    assert got["n_removed"] == 1 and r.g.rollingVoxelMap()[0].tolist() == [[20, 20, 20]]
    r.close()


def test_a_table_just_rebuilt_at_twice_the_size(ng):
    r = Ray(ng, 1.0)
    r.set_map(_block(-4, 4)[:30])
    assert r.g.voxelRollingStats()["table_slots"] == 64
    new = (_block(-4, 4)[40:46] + 0.5).astype(np.float32)
    r.source(new); r.prod.setSourceCovariances(_spd(len(new), 6))
    assert r.g.insertIntoVoxelMap(r.prod, I4) == (6, 6)
    assert r.g.voxelRollingStats()["table_slots"] == 128
    _raises(ng, ERR_STATE, r.g.voxelMapRayCounts)
    got, want = r.clear(_cube(200, 8.0, 7), I4, np.array([-3.5, -3.5, -3.5], np.float32), "behind a table rebuild", radius_cells=0.0, min_miss=1, back_cells=0)
    assert 0 < got["n_removed"] < 36
    r.close()


def _hash(keys, mask):
    k = np.asarray(keys, np.uint64)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    k = k ^ (k >> np.uint64(33))
    return (k & np.uint64(0xffffffff)).astype(np.int64) & mask


def test_a_table_with_long_probe_chains(ng):
    """24 voxels whose keys all hash to one slot of the 64-slot table (csrc/ngicp_voxel.h voxel_hash): the last of them is found behind
    23 others, and every empty cell whose hash falls into the run is refused only at its end."""
    cand = _block(-12, 12)
    home = _hash(ray.pack(cand), 63)
    cells = cand[home == 7][:24]
    assert len(cells) == 24
    r = Ray(ng, 1.0)
    r.set_map(cells)
    assert r.g.voxelRollingStats()["table_slots"] == 64
    centres = (cells + 0.5).astype(np.float32)
    o = np.array([0.5, 0.5, 0.5], np.float32)
    q = np.r_[centres, (o + 1.6 * (centres - o)).astype(np.float32), _cube(150, 12.0, 8)]
    got, want = r.clear(q, I4, o, "long chains, counted", dry_run=1, radius_cells=0.0, back_cells=0)
    assert (want["hit"] >= 1).all() and want["occupied"] >= 10
    got, want = r.clear(q[24:], I4, o, "long chains, removed", radius_cells=0.0, back_cells=0, min_miss=1)
    assert got["n_removed"] >= 5
    got, want = r.clear(q, I4, o, "the rebuilt table", dry_run=1, radius_cells=0.0, back_cells=0)
    r.close()


def test_the_radius_is_inclusive_and_measured_from_the_line(ng):
    res = 0.5
    r = Ray(ng, res)
    rad = 0.25 * res  # 0.125: exact, and so are the coordinates below
    ijk = np.array([[3, 0, 0], [5, 0, 0], [7, 0, 0], [9, 0, 0], [11, 1, 0]])
    mean = np.array([[1.75, 0.25 + rad, 0.25], [2.75, 0.25, np.nextafter(0.25 + rad, 1.0)], [3.75, 0.25 - rad, 0.25], [4.75, 0.25, 0.25 - 0.2],
                     [5.75, 0.75, 0.25]])
    r.set_map(ijk, mean)
    o, q = np.array([0.25, 0.25, 0.25], np.float32), np.array([[9.25, 0.25, 0.25], [9.25, 0.25, 0.25], [-4.25, 0.25, 0.25]], np.float32)
    got, want = r.clear(q, I4, o, "exactly r counts, the next double does not", dry_run=1)
    assert want["miss"].tolist() == [2, 0, 2, 0, 0]
    got, want = r.clear(q, I4, o, "the cell test alone", dry_run=1, radius_cells=0.0)
    assert want["miss"].tolist() == [2, 2, 2, 2, 0]
    got, want = r.clear(q, I4, o, "radius 0.5", dry_run=1, radius_cells=0.5)
    assert want["miss"].tolist() == [2, 2, 2, 2, 0]
    got, want = r.clear(q, I4, o, "radius 1.5 reaches no voxel whose cell the ray does not enter", dry_run=1, radius_cells=1.5)
    assert want["miss"].tolist() == [2, 2, 2, 2, 0]
    r.close()


# ---- the removal rule ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inserted(ng):
    """a map of two inserts (stamps 1 and 2) with real covariance sums, its state, and a scan whose rays cross it and partly end in it"""
    r = Ray(ng, 1.0)
    for k, (n, off) in enumerate(((700, (0.0, 0.0, 0.0)), (300, (2.5, 0.0, 0.0)))):
        pts = _cube(n, 3.0, 20 + k, off)
        r.source(pts); r.prod.setSourceCovariances(_spd(n, 30 + k))
        r.g.insertIntoVoxelMap(r.prod, T_RIGID)
    state = (*r.g.rollingVoxelMap(), r.g.voxelRollingStats()["inserts"])
    g = np.random.default_rng(9)
    d = g.normal(size=(500, 3))
    shell = (d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(5.0, 9.0, (500, 1))).astype(np.float32)
    scan = np.ascontiguousarray(np.r_[shell, _cube(60, 2.5, 12)])
    yield r, state, scan
    r.close()


@pytest.mark.parametrize("opt", [dict(min_miss=1), dict(min_miss=2), dict(min_miss=5), dict(min_miss=1, keep_stamp=2), dict(min_miss=2, radius_cells=0.25)],
                         ids=lambda o: " ".join(f"{k}={v}" for k, v in o.items()))
def test_removal_rule(ng, inserted, opt):
    r, state, scan = inserted
    o = np.array([-6.0, 0.5, 0.3], np.float32)
    opt = {"radius_cells": 0.0, **opt}
    r.g.setRollingVoxelMap(*state)
    got, want = r.clear(scan, I4, o, str(opt), **opt)
    miss, hit, keep, stamp = want["miss"], want["hit"], want["keep"], state[4]
    print(f"{opt}: {len(keep)} voxels, {got['n_removed']} removed, {int(((miss >= opt['min_miss']) & (hit > 0)).sum())} kept by a hit")
    assert 0 < got["n_removed"] < len(keep)
    assert ((miss >= opt["min_miss"]) & (hit == 1)).any() and keep[(hit > 0)].all()  # misses and one hit: stays
    assert (miss[keep & (hit == 0) & (stamp < opt.get("keep_stamp", 3))] < opt["min_miss"]).all()
    if "keep_stamp" in opt:
        assert ((miss >= 1) & (hit == 0) & (stamp == 2)).any() and keep[stamp == 2].all()  # the last insert's voxels are protected
    _, _, _, _, st_after = r.g.rollingVoxelMap()
    assert np.array_equal(st_after, stamp[keep]) and r.g.voxelRollingStats()["inserts"] == 2
    # the passes read the rebuilt table: the handle equals a fresh one restored from the model's state, bit for bit
    fresh = ng.NanoGICP()
    fresh.setVoxelResolution(1.0); fresh.setVoxelRolling(True)
    fresh.setRollingVoxelMap(*[a[keep] for a in state[:5]], state[5])
    src = clouds.transform_points(T_RIGID, _cube(800, 3.0, 20)[:500])
    cs = _spd(len(src), 41)
    guess = clouds.make_pose((0.05, -0.03, 0.02), (0.3, -0.2, 0.5)).astype(np.float32)
    out = []
    for e in (r.g, fresh):
        e.setInputSource(src, identity=0); e.setSourceCovariances(cs)
        fit = e.voxelFitness(T=guess)
        e.align(guess)
        out.append((np.array([fit["mahalanobis"], fit["sqdist"], fit["n_inliers"], fit["n_matched"]]), e.getFinalTransformation().copy(), e.getFinalHessian().copy(),
                    e.lm_trace().copy(), e.voxel_correspondences(), np.array([e.nr_iterations_, int(e.converged_)])))
    for i, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(a, b), f"item {i} on the cleared handle differs from the restored one"
    assert out[0][0][3] > 100 and (out[0][4] >= 0).any()
    fresh.close()


def test_a_clear_that_removes_everything_leaves_a_map_an_insert_refills(ng):
    r = Ray(ng, 1.0)
    r.set_map([[2, 0, 0], [3, 0, 0], [5, 0, 0]], stamp=[1, 2, 3])
    q = np.tile(np.array([[9.5, 0.5, 0.5]], np.float32), (3, 1))
    got, want = r.clear(q, I4, O, "everything goes")
    assert got["n_removed"] == 3 and r.g.voxelRollingStats()["n_vox"] == 0 and len(r.g.voxelMapRayCounts()[0]) == 3
    got, want = r.clear(q, I4, O, "an empty map")
    assert (got["n_removed"], got["occupied"], got["misses"]) == (0, 0, 0) and got["steps"] == 3 * 6 and len(r.g.voxelMapRayCounts()[0]) == 0
    pts = _cube(200, 2.0, 13)
    r.source(pts); r.prod.setSourceCovariances(_spd(200, 14))
    n_new, n_touched = r.g.insertIntoVoxelMap(r.prod, I4)
    ijk, S, C, cnt, st = r.g.rollingVoxelMap()
    assert n_new == n_touched == len(ijk) > 20 and (st == 4).all() and cnt.sum() == 200  # the counter carried on: 3 inserts before
    got, want = r.clear(q, I4, O, "the refilled map", radius_cells=0.0, min_miss=1, back_cells=0)
    assert got["occupied"] > 0
    r.close()


# ---- dry run, refusals, states, determinism --------------------------------------------------------------------------------------------
def test_a_dry_run_leaves_the_map_the_stats_and_the_hooks_alone(ng, inserted):
    r, state, scan = inserted
    o = np.array([-6.0, 0.5, 0.3], np.float32)
    r.g.setRollingVoxelMap(*state)
    src = clouds.transform_points(T_RIGID, _cube(800, 3.0, 20)[:500])  # (the cloud test_removal_rule aligns: one source size per handle)
    r.g.setInputSource(src, identity=0); r.g.setSourceCovariances(_spd(len(src), 41))
    T = np.eye(4)
    H, b, e = r.g.linearize(T)
    err0, corr0 = r.g.compute_error(T), r.g.voxel_correspondences()
    drop = lambda s: {k: v for k, v in s.items() if not k.endswith("_ms")}
    before, vm0, stats0 = r.g.rollingVoxelMap(), r.g.voxelMap(), r.g.voxelRollingStats()
    got, want = r.clear(scan, I4, o, "dry run", dry_run=1, radius_cells=0.0, min_miss=1)
    assert got["n_removed"] == 0 and ((want["miss"] >= 1) & (want["hit"] == 0)).any()
    for a, c in zip(before + vm0, r.g.rollingVoxelMap() + r.g.voxelMap()):
        assert np.array_equal(a, c)
    assert drop(r.g.voxelRollingStats()) == drop(stats0)
    assert r.g.compute_error(T) == err0 and np.array_equal(r.g.voxel_correspondences(), corr0)  # the hooks' state is still there
    got, want = r.clear(scan, I4, o, "the same for real", radius_cells=0.0, min_miss=1)
    assert got["n_removed"] > 0
    _raises(ng, ERR_STATE, r.g.compute_error, T)  # ... and dropped by the call that removes


def test_refusals_and_states(ng):
    r = Ray(ng, 1.0)
    _raises(ng, ERR_STATE, r.g.voxelMapRayCounts)  # before any call
    r.set_map(_block(-3, 3), stamp=np.arange(216) % 3 + 1)
    q = _cube(100, 6.0, 15)
    fresh_producer = ng.NanoGICP()
    _raises(ng, ERR_ARG, r.g.clearVoxelMapAlongRays, fresh_producer, I4)  # a producer without a source
    _raises(ng, ERR_STATE, r.g.voxelMapRayCounts)
    got, want = r.clear(q, I4, O, "the accepted call", dry_run=1, radius_cells=0.0)
    state = r.g.rollingVoxelMap(), r.g.voxelRollingStats()["inserts"], r.g.voxelMap()

    def unchanged(label):
        now = r.g.rollingVoxelMap(), r.g.voxelRollingStats()["inserts"], r.g.voxelMap()
        for a, b in zip(state[0] + state[2], now[0] + now[2]):
            assert a.tobytes() == b.tobytes(), f"{label}: the map changed"
        assert now[1] == state[1], label
        miss, hit = r.g.voxelMapRayCounts()  # the counts of the accepted call are still readable
        assert np.array_equal(miss, want["miss"]) and np.array_equal(hit, want["hit"]), label

    far = q.copy(); far[57] = (1.0e7, 0.0, 0.0)
    T_nan = I4.copy(); T_nan[1, 3] = np.nan
    refusals = [("a point at 1e7 m", far, I4, O, {}), ("a NaN point", q, T_nan, O, {}), ("an origin without a cell", q, I4, (0.0, -3.0e6, 0.0), {}),
                ("a NaN origin", q, T_nan, None, {}), ("an infinite origin", q, I4, (np.inf, 0.0, 0.0), {})]
    refusals += [(f"{k} = {v}", q, I4, O, {k: v}) for k, v in (("near_cells", 0), ("back_cells", -1), ("max_steps", 0), ("max_steps", 65537), ("min_miss", 0),
                                                               ("radius_cells", -0.1), ("radius_cells", float("nan")))]
    for label, pts, T, o, opt in refusals:
        r.source(pts)
        _raises(ng, ERR_ARG, r.g.clearVoxelMapAlongRays, r.prod, T, o, **{"min_miss": 1, "radius_cells": 0.0, **opt})  # (accepted, it would remove)
        if not opt:
            with pytest.raises(ray.Refused):
                r.model(pts, T, o)
        unchanged(label)
    with pytest.raises(TypeError):
        r.g.clearVoxelMapAlongRays(r.prod, I4, O, no_such_option=1)
    r.source(q)
    r.g.setVoxelRolling(False)
    _raises(ng, ERR_STATE, r.g.clearVoxelMapAlongRays, r.prod, I4, O)  # the rolling setting off
    r.g.setVoxelRolling(True)
    unchanged("the setting off and on again")
    got2, want2 = r.clear(q, I4, O, "max_steps = 65536 is accepted", dry_run=1, max_steps=65536)
    # anything else that writes the map ends the counts' validity: an insert, an eviction, a restore
    r.prod.setSourceCovariances(_spd(len(q), 16))
    r.g.insertIntoVoxelMap(r.prod, I4)
    _raises(ng, ERR_STATE, r.g.voxelMapRayCounts)  # after an insert
    r.clear(q, I4, O, "counted again", dry_run=1)
    r.g.evictVoxelMap((0.0, 0.0, 0.0), 100.0, 0)
    _raises(ng, ERR_STATE, r.g.voxelMapRayCounts)
    r.g.setVoxelResolution(0.0)
    _raises(ng, ERR_STATE, r.g.clearVoxelMapAlongRays, r.prod, I4, O)  # res = 0
    fresh_producer.close(); r.close()


def test_two_runs_on_two_handles_are_bit_equal(ng, inserted):
    r0, state, scan = inserted
    o = np.array([-6.0, 0.5, 0.3], np.float32)
    out = []
    for _ in range(2):
        r = Ray(ng, 1.0)
        r.g.setRollingVoxelMap(*state)
        r.source(scan)
        res = r.g.clearVoxelMapAlongRays(r.prod, T_RIGID, o, min_miss=1)
        out.append((*r.g.voxelMapRayCounts(), np.array([res[k] for k in TOTALS]), *r.g.rollingVoxelMap(), *r.g.voxelMap()))
        r.close()
    assert out[0][2][3] > 0
    for i, (a, b) in enumerate(zip(*out)):
        assert a.tobytes() == b.tobytes(), f"item {i}"


# ---- the drive, end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1.0, 0.5])
def test_the_drive_clears_the_moving_box_and_keeps_the_room(ng, res):
    """Frames 0 .. 6 of the room with a moving box inserted at their poses with the engine's own covariances; frame 7 clears before it is
    inserted.  The engine equals the model exactly; the MODEL's numbers meet the conditions (>= 85 % of the trail, <= 1 % of the static
    voxels with the defaults; the cell test alone removes more than ten times as many static voxels)."""
    frames = drive.frames()
    r = Ray(ng, res)
    for pose, pts, _ in frames[:7]:
        r.source(pts)
        r.g.insertIntoVoxelMap(r.prod, pose)
    state = (*r.g.rollingVoxelMap(), r.g.voxelRollingStats()["inserts"])
    trail = drive.trail_mask(state[0], res)
    pose, pts, _ = frames[7]
    if res == 1.0:
        got0, want0 = r.clear(pts, pose, None, "the cell test alone", radius_cells=0.0)
        _, _, st0, _ = drive.report(f"{res} m, radius_cells = 0", want0, trail)
        r.g.setRollingVoxelMap(*state)
    got, want = r.clear(pts, pose, None, "defaults")
    tr, n_trail, st, n_static = drive.report(f"{res} m, defaults", want, trail)
    print(f"  the counting kernel: {got['kernel_ms']:.3f} ms for {len(pts)} rays on {len(trail)} voxels")
    assert n_trail >= 20 and tr >= 0.85 * n_trail and st <= 0.01 * n_static
    if res == 1.0:
        assert st0 > 10 * st
    r.source(pts)
    n_new, _ = r.g.insertIntoVoxelMap(r.prod, pose)  # the frame loop carries on: clear, then insert
    assert n_new > 0 and r.g.voxelRollingStats()["inserts"] == 8
    r.close()
