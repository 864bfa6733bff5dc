"""The numpy model of the voxel pose search (tests/_pose_search_model.py) held to the definition spelled as a loop, and - before any
engine is asked - to the end-to-end margins tests/test_gpu_pose_search.py relies on: on the scan-context fixtures the lattice point
nearest the truth wins by a wide lead."""
import numpy as np
import pytest

import _pose_search_cases as pc
import _pose_search_model as psm

F = np.float32


def _random_case(seed, n, n_map, spread=3.0):
    rng = np.random.default_rng(seed)
    src = rng.uniform(-spread, spread, (n, 3)).astype(F)
    map_ijk = np.unique(rng.integers(-7, 8, (n_map, 3)), axis=0)
    Ts = psm.yaw_lattice(np.eye(4), 3, 0.7)
    Ts[1, :3, 3] = (0.3, -0.2, 0.1)
    return Ts, src, map_ijk


@pytest.mark.parametrize("extent", [(0, 0, 0), (1, 0, 0), (3, 2, 1), (0, 5, 2)])
@pytest.mark.parametrize("sparse", [False, True])
def test_the_vectorised_model_is_the_naive_loop(extent, sparse):
    Ts, src, map_ijk = _random_case(1, 41, 300)
    src[5] = src[6]                      # duplicates count each time
    src[7, 1] = np.nan                   # no cell
    src[8, 0] = F(2.0 ** 20 * 0.5)       # at 2^20 cells: no cell
    want = psm.naive_volume(Ts, src, map_ijk, 0.5, extent)
    got = psm.score_volume(Ts, src, map_ijk, 0.5, extent, force_sparse=sparse)
    assert got.dtype == np.int32 and got.shape == (3, 2 * extent[2] + 1, 2 * extent[1] + 1, 2 * extent[0] + 1)
    assert np.array_equal(got, want)
    assert want.sum() > 0


def test_cells_next_to_the_key_range_lose_the_shifts_that_leave_it():
    lim = psm.VOXEL_LIMIT
    map_ijk = np.array([[lim - 1, 0, 0], [lim - 2, 0, 0], [-(lim - 1), 3, 0]])
    src = np.array([[(lim - 1.5) * 0.5, 0.1, 0.1], [-(lim - 1.5) * 0.5, 1.6, 0.1]], dtype=F)  # cells (lim - 2, 0, 0) and (-(lim - 1), 3, 0)
    Ts = np.eye(4, dtype=F)[None]
    ijk, has = psm.cells(Ts[0], src, 0.5)
    assert has.all() and ijk.tolist() == [[lim - 2, 0, 0], [-(lim - 1), 3, 0]]
    for sparse in (False, True):
        got = psm.score_volume(Ts, src, map_ijk, 0.5, (2, 0, 0), force_sparse=sparse)
        assert np.array_equal(got, psm.naive_volume(Ts, src, map_ijk, 0.5, (2, 0, 0)))
        assert got[0, 0, 0].tolist() == [0, 0, 2, 1, 0]  # sx = +2 would be cell 2^20: outside the range, and in no map


def test_ranking_breaks_ties_by_pose_then_shift_index():
    vol = np.zeros((2, 1, 3, 3), dtype=np.int32)
    vol[1, 0, 0, 2] = vol[0, 0, 2, 1] = vol[0, 0, 1, 0] = 5
    vol[1, 0, 1, 1] = 9
    pose, shift, score = psm.ranking(vol, 6)
    assert score.tolist() == [9, 5, 5, 5, 0, 0]
    assert pose.tolist() == [1, 0, 0, 1, 0, 0]
    assert shift.tolist() == [[0, 0, 0], [-1, 0, 0], [0, 1, 0], [1, -1, 0], [-1, -1, 0], [0, -1, 0]]
    assert len(psm.ranking(vol, 64)[0]) == 18  # top_k beyond B |S|
    assert psm.shift_index((1, -1, 0), (1, 1, 0)) == 2


def test_candidate_pose_and_lattice():
    T = psm.yaw_lattice(np.eye(4), 72, np.radians(5.0))[7]
    T[:3, 3] = (0.25, -3.0, 1e-3)
    got = psm.candidate_pose(T, (5, -3, 1), 0.5)
    assert got.dtype == F and np.array_equal(got[:3, :3], T[:3, :3])
    assert got[:3, 3].tolist() == [F(2.75), F(-4.5), F(np.float64(F(1e-3)) + 0.5)]
    assert np.allclose(T[:2, :2], [[np.cos(np.radians(35)), -np.sin(np.radians(35))], [np.sin(np.radians(35)), np.cos(np.radians(35))]], atol=1e-7)


@pytest.mark.parametrize("move", pc.MOVES)
def test_the_model_alone_finds_the_revisit(move):
    """72 yaws x 25 x 25 x 3 shifts at 0.5 m: the best candidate is (35 degrees, round(move / res)) and leads the runner-up by >= 50."""
    pose, shift, score = pc.model_top(move)
    print(f"move {move}: best {score[0]} at {5 * pose[0]} deg {shift[0].tolist()}, runner-up {score[1]} at {5 * pose[1]} deg {shift[1].tolist()}")
    assert 5 * int(pose[0]) == 35
    assert shift[0].tolist() == [round(move[0] / pc.RES), round(move[1] / pc.RES), 0]
    assert int(score[0]) - int(score[1]) >= 50
