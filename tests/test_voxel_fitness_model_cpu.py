"""The numpy model of the voxel fitness (tests/_voxel_fitness_model.py; include/ngicp.h "voxel fitness") proves itself on the properties
of the definition, and the fixtures the GPU tests use (tests/test_gpu_voxel_fitness.py) are shown to be ones on which a comparison with
the engine cannot hide a failure: no gate lies within 1e-6 (relative) of a per-point term, and no point's best two slots lie within 1e-6
of each other - so a rounding difference can neither move a point across a gate nor change a winner, and no point has to be exempted."""
import numpy as np
import pytest

import _vgicp_model as vm
import _vgicp_nbr_model as nm
import _vgicp_rolling_model as rm
import _voxel_fitness_model as fm

DBL_MAX = fm.DBL_MAX


@pytest.fixture(scope="module")
def tgt_map():
    pts, covs = fm.target()
    return vm.VoxelMap(pts, covs, fm.RES)


@pytest.fixture(scope="module")
def values(tgt_map):
    """point_values of every (size, pose, K) of the GPU comparison, computed once"""
    out = {}
    for n in fm.SIZES:
        src, cs = fm.source(n)
        for name, T in fm.POSES.items():
            for K in fm.NEIGHBORS:
                out[n, name, K] = fm.point_values(src, cs, tgt_map, T, K)
    return out


def test_the_engine_s_routines_are_spelled_right():
    """the spelled-out rotation, inverse and quadratic form against numpy's own, on random SPD input"""
    C = fm.spd(50, 1)[:, :3, :3]
    R = fm.pose((0, 0, 0), (10.0, -20.0, 30.0))[:3, :3].astype(np.float64)
    full = lambda s: np.stack([s[:, [0, 1, 2]], s[:, [1, 3, 4]], s[:, [2, 4, 5]]], axis=1)
    assert np.allclose(full(fm.rotate_sym6(R, fm.sym6(C))), R @ C @ R.T, rtol=1e-12, atol=1e-15)
    assert np.allclose(full(fm.inv3_sym6(fm.sym6(C))), np.linalg.inv(C), rtol=1e-9)
    e = np.random.default_rng(2).normal(0, 1, (50, 3))
    assert np.allclose(fm.err_term(e, fm.sym6(C)), np.einsum("ni,nij,nj->n", e, C, e), rtol=1e-12)
    assert np.array_equal(fm.rotate_sym6(R, fm.sym6(C))[7], fm.sym6(rm.rotate_sym(R, C[7])[None])[0])  # the rolling model's spelling, bit for bit


def test_a_cloud_scored_at_identity_on_its_own_map_is_fully_matched(tgt_map):
    pts, covs = fm.target()
    for K in fm.NEIGHBORS:
        m, d, v, matched, _ = fm.point_values(pts, covs, tgt_map, np.eye(4, dtype=np.float32), K)
        assert matched.all() and (v >= 0).all() and (m >= 0).all() and np.isfinite(m).all()
        s = fm.score(pts, covs, tgt_map, np.eye(4, dtype=np.float32), K)
        assert s["n_matched"] == s["n_inliers"] == len(pts) and s["mahalanobis"] < DBL_MAX
    # DIRECT1: every point's voxel is its own, and a voxel of count 1 explains its only point exactly
    m, d, v, _, _ = fm.point_values(pts, covs, tgt_map, np.eye(4, dtype=np.float32), 1)
    assert np.array_equal(v, tgt_map.lookup(pts))
    alone = tgt_map.count[v] == 1
    assert alone.any() and (m[alone] == 0).all() and (d[alone] == 0).all()


def test_a_wider_neighbourhood_never_scores_a_point_worse(values):
    """the slots of DIRECT1 are among DIRECT7's, and those among DIRECT27's: the best term can only fall"""
    seen = 0
    for n in fm.SIZES:
        for name in fm.POSES:
            m1, m7, m27 = (values[n, name, K] for K in fm.NEIGHBORS)
            on1, on7 = m1[3], m7[3]
            assert (m7[3] | ~on1).all() and (m27[3] | ~on7).all()  # matched under the narrower one: matched under the wider one
            assert (m7[0][on1] <= m1[0][on1]).all() and (m27[0][on7] <= m7[0][on7]).all()
            seen += int(on1.sum())
    assert seen > 500


def test_a_pose_two_to_the_twenty_voxels_away_matches_nothing(tgt_map):
    src, cs = fm.source(257)
    for K in fm.NEIGHBORS:
        for far in (2.0 ** 20 * fm.RES, -(2.0 ** 20) * fm.RES - 8.0, 3e9):
            T = fm.pose((far, 0.0, 0.0))
            s = fm.score(src, cs, tgt_map, T, K)
            assert s == {"mahalanobis": DBL_MAX, "sqdist": DBL_MAX, "n_inliers": 0, "n_matched": 0}, (K, far)
            m, d, v, matched, _ = fm.point_values(src, cs, tgt_map, T, K)
            assert not matched.any() and (m == -1).all() and (d == -1).all() and (v == -1).all()


def test_the_gate_is_monotone(tgt_map):
    src, cs = fm.source(700)
    for K in fm.NEIGHBORS:
        prev = -1
        for gate in (0.0, 0.1, 1.0, 2.5, 10.0, 40.0, 1e3, DBL_MAX):
            s = fm.score(src, cs, tgt_map, fm.POSES["small"], K, gate)
            assert s["n_inliers"] >= prev and s["n_inliers"] <= s["n_matched"]
            prev = s["n_inliers"]
        assert prev == s["n_matched"] > 0  # no gate: every matched point with a finite term counts


def test_a_whole_voxel_shift_of_map_and_pose_leaves_the_counts(tgt_map):
    """The records moved by k voxels (ijk + k, mean + k res) and the pose's translation by the same k res: every point lands in the moved
    voxel of the one it was in.  Source coordinates and the translation are multiples of 2^-10, so that the float sums are exact."""
    src, cs = fm.source(257)
    src = (np.round(src * 1024) / 1024).astype(np.float32)
    k = np.array([4, -6, 2])
    moved = fm.RecordMap(fm.RES, tgt_map.ijk + k, (tgt_map.mean + k * fm.RES) * tgt_map.count[:, None], tgt_map.cov * tgt_map.count[:, None, None], tgt_map.count)
    T0, T1 = fm.pose((0.25, -0.5, 0.125)), fm.pose((0.25, -0.5, 0.125) + k * fm.RES)
    for K in fm.NEIGHBORS:
        for gate in (2.5, DBL_MAX):
            a, b = fm.score(src, cs, tgt_map, T0, K, gate), fm.score(src, cs, moved, T1, K, gate)
            assert (a["n_matched"], a["n_inliers"]) == (b["n_matched"], b["n_inliers"]) and a["n_matched"] > 0, (K, gate)
            assert abs(a["mahalanobis"] - b["mahalanobis"]) <= 1e-9 * a["mahalanobis"]
        va, vb = fm.point_values(src, cs, tgt_map, T0, K)[2], fm.point_values(src, cs, moved, T1, K)[2]
        assert np.array_equal(va, vb)  # (the numbering moved with the records)


def test_a_nan_term_never_wins_and_a_point_without_a_winner_counts_as_matched():
    """one voxel whose covariance makes cov_v + R C_a R^T singular to the last bit (det == 0: M is inf / NaN)"""
    pts = np.array([[0.25, 0.25, 0.25], [1.25, 0.25, 0.25]], np.float32)
    covs = np.zeros((2, 4, 4))
    covs[1, :3, :3] = np.eye(3)
    m = vm.VoxelMap(pts, covs, 1.0)
    src, cs = np.array([[0.5, 0.5, 0.5]], np.float32), np.zeros((1, 4, 4))
    mm, d, v, matched, _ = fm.point_values(src, cs, m, np.eye(4, dtype=np.float32), 1)
    assert matched[0] and mm[0] == np.inf and d[0] == np.inf and v[0] == -1
    s = fm.score(src, cs, m, np.eye(4, dtype=np.float32), 1)
    assert s["n_matched"] == 1 and s["n_inliers"] == 0 and s["mahalanobis"] == DBL_MAX
    mm, d, v, matched, _ = fm.point_values(src, cs, m, np.eye(4, dtype=np.float32), 7)  # slot 1 (+x) is the sound voxel
    assert matched[0] and np.isfinite(mm[0]) and v[0] == 1


# ---- the fixtures of the GPU comparison ------------------------------------------------------------------------------------------------------
def test_the_fixtures_keep_every_gate_and_every_runner_up_at_a_distance(values):
    worst_gate, worst_gap, unmatched, multi = np.inf, np.inf, 0, 0
    for key, (m, d, v, matched, slot_m) in values.items():
        worst_gate = min(worst_gate, fm.gate_margin(m[matched], fm.GATES))
        worst_gap = min(worst_gap, fm.slot_gap(slot_m))
        unmatched += int((~matched).sum())
        multi += int((np.isfinite(slot_m).sum(axis=1) >= 2).sum())
    print(f"closest gate: {worst_gate:.2e} relative; closest runner-up: {worst_gap:.2e} relative; {unmatched} unmatched values, {multi} with two or more slots")
    assert worst_gate >= 1e-6 and worst_gap >= 1e-6
    assert unmatched > 0 and multi > 1000  # both kinds of point are there to be compared


@pytest.mark.parametrize("kind", ["target", "merged", "rolling"])
def test_the_map_kinds_fixtures_keep_their_distance_too(kind):
    m = fm.kind_map(kind)
    src, cs = fm.kind_source()
    for K in fm.NEIGHBORS:
        for T in fm.POSES.values():
            mm, d, v, matched, slot_m = fm.point_values(src, cs, m, T, K)
            assert fm.gate_margin(mm[matched], fm.GATES) >= 1e-6 and fm.slot_gap(slot_m) >= 1e-6, (kind, K)
            assert 0 < matched.sum() < len(src)
    if kind == "rolling":
        assert isinstance(m, rm.RollingVoxelMap) and m.inserts == 2
    assert nm.lookup_slots(m, src, 1).shape == (len(src), 1)
