"""The numpy model of the clearing along rays (tests/_vgicp_ray_model.py) proves itself on the CPU: the walk has N steps, is 6-connected
and ends at c1; it visits every cell a dense sampling of the segment falls into; ties go x before y before z; and the counting rules
(near / back / max_steps, the radius, hit) on maps small enough to count by hand."""
import numpy as np
import pytest

import _vgicp_ray_model as ray

RESOLUTIONS = (1.0, 0.5, 0.3)


def _random_rays(res, n, seed):
    g = np.random.default_rng(seed)
    o = g.uniform(-3, 3, 3).astype(np.float32)
    direction = g.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    q = (o + direction * g.uniform(0.2, 25.0, (n, 1)) * min(1.0, 2 * res)).astype(np.float32)
    return o, q


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_the_walk_has_N_steps_is_6_connected_and_ends_at_c1(res):
    o, q = _random_rays(res, 400, 11)
    r = ray.Rays(o, q, res)
    cells = r.full_walk()
    assert np.array_equal(r.N, np.abs(r.c1 - r.c0).sum(axis=1)) and r.N.max() > 20
    assert (cells[:, 0] == r.c0).all()
    assert np.array_equal(cells[np.arange(len(q)), r.N], r.c1)
    step = np.abs(np.diff(cells, axis=1)).sum(axis=2)  # 1 for a step, 0 behind the ray's end
    assert np.array_equal(step.sum(axis=1), r.N)
    assert ((step == 1) == (np.arange(1, cells.shape[1])[None, :] <= r.N[:, None])).all()


def test_every_cell_of_a_dense_sampling_is_visited():
    visited_total = unseen_total = 0
    t = np.linspace(0.0, 1.0, 20001)[:, None]
    for res in RESOLUTIONS:
        o, q = _random_rays(res, 400, 23)
        r = ray.Rays(o, q, res)
        cells = r.full_walk()
        for i in range(len(q)):
            visited = np.unique(ray.pack(cells[i, :r.N[i] + 1]))
            sampled = np.unique(ray.pack(np.floor((r.od + t * r.d[i]) / np.float64(res)).astype(np.int64)))
            assert np.isin(sampled, visited).all(), f"res {res}, ray {i}: a sampled cell is not visited"
            visited_total += len(visited)
            unseen_total += len(visited) - len(sampled)
    share = unseen_total / visited_total
    print(f"{visited_total} visited cells over {3 * 400} rays, {unseen_total} of them not seen by the sampling ({100 * share:.3f} %)")
    assert share <= 0.005


@pytest.mark.parametrize("sign", [1, -1])
def test_ties_on_exact_corner_diagonals_go_x_then_y_then_z(sign):
    o = np.array([0.5, 0.5, 0.5], np.float32)
    q = o + sign * np.array([[3, 3, 3], [2, 2, 0], [0, 2, 2], [2, 0, 2]], np.float32)
    r = ray.Rays(o, q, 1.0)
    cells = r.full_walk()
    axes = [[int(np.flatnonzero(cells[i, j] != cells[i, j - 1])[0]) for j in range(1, r.N[i] + 1)] for i in range(len(q))]
    assert axes == [[0, 1, 2] * 3, [0, 1] * 2, [1, 2] * 2, [0, 2] * 2]


def test_counting_rules_on_a_straight_ray():
    """One ray along +x through ten occupied cells 0 .. 9 (the origin in cell 0, the end in cell 9): steps 1 .. 8 lie between them."""
    ijk = np.array([[i, 0, 0] for i in range(10)])
    mean = ijk + 0.5
    o, q = np.array([0.5, 0.5, 0.5], np.float32), np.array([[9.5, 0.5, 0.5]], np.float32)
    c = ray.ray_counts(ijk, mean, 1.0, q, o, near_cells=1, back_cells=0)
    assert c["miss"].tolist() == [0] + [1] * 8 + [0] and c["hit"].tolist() == [0] * 9 + [1] and (c["steps"], c["occupied"], c["misses"]) == (8, 8, 8)
    c = ray.ray_counts(ijk, mean, 1.0, q, o)  # the defaults: near 1, back 2
    assert c["miss"].tolist() == [0] + [1] * 6 + [0] * 3 and c["steps"] == 6
    c = ray.ray_counts(ijk, mean, 1.0, q, o, near_cells=3, back_cells=0, max_steps=5)
    assert c["miss"].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0] and c["hit"][9] == 1 and c["steps"] == 3
    c = ray.ray_counts(ijk, mean, 1.0, q[:, :] * 0 + np.float32(0.75), o)  # inside one cell: N = 0
    assert c["miss"].sum() == 0 and c["hit"].tolist() == [1] + [0] * 9 and c["steps"] == 0


def test_the_radius_is_inclusive_and_measured_from_the_line():
    ijk = np.array([[3, 0, 0], [4, 0, 0], [5, 0, 0]])
    mean = np.array([[3.5, 0.5 + 0.25, 0.5], [4.5, 0.5, np.nextafter(0.75, 1.0)], [5.5, 0.5, 0.5]])
    o, q = np.array([0.5, 0.5, 0.5], np.float32), np.array([[9.5, 0.5, 0.5]], np.float32)
    assert ray.ray_counts(ijk, mean, 1.0, q, o, radius_cells=0.25)["miss"].tolist() == [1, 0, 1]
    assert ray.ray_counts(ijk, mean, 1.0, q, o, radius_cells=0.0)["miss"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("res", [1.0, 0.5])
def test_the_drive_on_the_numpy_map_clears_the_trail_and_keeps_the_room(res):
    """The drive of tests/test_gpu_vgicp_ray.py on a map summed in numpy: with the defaults at least 85 % of the moving box's trail goes
    and at most 1 % of the static voxels; the cell test alone removes more than ten times as many static voxels."""
    import _vgicp_ray_drive as drive
    ijk, mean, stamp = drive.numpy_map(res)
    trail = drive.trail_mask(ijk, res)
    pose, pts, _ = drive.frames()[7]
    tr, n_trail, st, n_static = drive.report(f"{res} m, defaults", ray.ray_clear(ijk, mean, stamp, res, pts, pose), trail)
    assert n_trail >= 20 and tr >= 0.85 * n_trail and st <= 0.01 * n_static
    if res == 1.0:
        _, _, st0, _ = drive.report(f"{res} m, the cell test alone", ray.ray_clear(ijk, mean, stamp, res, pts, pose, radius_cells=0.0), trail)
        assert st0 > 10 * st


def test_removal_rule_and_refusals():
    ijk = np.array([[2, 0, 0], [3, 0, 0], [9, 0, 0]])
    mean, stamp = ijk + 0.5, np.array([1, 2, 1])
    pts = np.array([[9.5, 0.5, 0.5], [9.5, 0.5, 0.5]], np.float32)
    T = np.eye(4, dtype=np.float32); T[:3, 3] = 0.5
    out = ray.ray_clear(ijk, mean, stamp, 1.0, pts - 0.5, T)
    assert out["miss"].tolist() == [2, 2, 0] and out["hit"].tolist() == [0, 0, 2] and out["keep"].tolist() == [False, False, True]
    assert ray.ray_clear(ijk, mean, stamp, 1.0, pts - 0.5, T, keep_stamp=2)["keep"].tolist() == [False, True, True]
    assert ray.ray_clear(ijk, mean, stamp, 1.0, pts - 0.5, T, min_miss=3)["n_removed"] == 0
    assert ray.ray_clear(ijk, mean, stamp, 1.0, pts - 0.5, T, dry_run=1)["keep"].all()
    for bad in (np.array([[1e7, 0, 0]], np.float32), np.array([[np.nan, 0, 0]], np.float32)):
        with pytest.raises(ray.Refused):
            ray.ray_clear(ijk, mean, stamp, 1.0, bad, T)
    with pytest.raises(ray.Refused):
        ray.ray_clear(ijk, mean, stamp, 1.0, pts, T, origin=(0, -3e6, 0))
