"""The voxel pose search on the GPU (ngicp_voxel_pose_search*; k_ps_map_box / k_ps_src_box / k_ps_occ_fill / k_ps_score / k_ps_topk in
csrc/ngicp_pose_search.h) against the numpy model of its definition (tests/_pose_search_model.py, which proves itself - and the
end-to-end fixtures used here - in test_pose_search_model_cpu.py).

Every score is an integer: volumes, rankings and candidate poses are compared with np.array_equal, nothing has a tolerance.  The one
bound on floats is the end-to-end test's: two exact alignments that reach the same fixed point end within twice the handle's epsilons
of each other (the bound tests/test_gpu_scan_context.py derives)."""
import os
import subprocess

import numpy as np
import pytest

import _pose_search_cases as pc
import _pose_search_model as psm
import _scan_context_cases as cs
import _voxel_fitness_model as fm
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -2, -3
F = np.float32
LIM = psm.VOXEL_LIMIT
EXTENTS = ((0, 0, 0), (1, 0, 0), (3, 2, 1), (31, 1, 0), (0, 31, 7))
I4 = np.eye(4, dtype=F)


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _raises(ng, code, fn, *a, **kw):
    with pytest.raises(ng.NgicpError) as e:
        fn(*a, **kw)
    assert e.value.code == code, f"{e.value}"


def _kind_engine(ng, kind):
    """tests/test_gpu_voxel_fitness.py's three kinds of map: the target's, the one merged from two keyframes, the rolling one after two
    inserts AND AN EVICTION (no target is ever set on that handle)"""
    (a, ca), (b, cb) = fm.kind_clouds()
    g, prod = ng.NanoGICP(), ng.NanoGICP()
    g.setVoxelResolution(fm.KIND_RES)
    if kind == "target":
        g.setInputTarget(np.r_[a, b]); g.setTargetCovariances(np.r_[ca, cb])
    elif kind == "merged":
        g.setVoxelSubmapMerge(True)
        for p, c in ((a, ca), (b, cb)):
            prod.setInputSource(p); prod.setSourceCovariances(c)
            g.addKeyframe(prod)
        g.setSubmapKeyframes([0, 1])
    else:
        g.setVoxelRolling(True)
        for (p, c), T in zip(((a, ca), (b, cb)), fm.ROLL_POSES):
            prod.setInputSource(p); prod.setSourceCovariances(c)
            g.insertIntoVoxelMap(prod, T)
        assert g.evictVoxelMap(fm.ROLL_EVICT[0], fm.ROLL_EVICT[1], 0) > 0
    prod.close()
    return g


def _custom(ng, ijk, res=0.5):
    """an engine whose rolling map holds exactly the cells `ijk` (one point in the middle of each)"""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    g = ng.NanoGICP()
    g.setVoxelResolution(res)
    g.setVoxelRolling(True)
    n = len(ijk)
    g.setRollingVoxelMap(ijk, (ijk + 0.5) * res, np.tile(np.eye(3) * 1e-2, (n, 1, 1)), np.ones(n, np.int32), np.ones(n, np.int64), 1)
    return g


def _centres(ijk, res=0.5):
    """float32 points in the middle of the given cells"""
    return ((np.asarray(ijk, np.float64) + 0.5) * res).astype(F)


def _check(g, Ts, src, map_ijk, res, extent, top_k=8, label=""):
    """one search against the model: the returned ranking, the candidate poses and the full volume"""
    Ts = np.asarray(Ts, F)
    want = psm.score_volume(Ts, src, map_ijk, res, extent)
    pose, shift, score, cand = g.voxelPoseSearch(Ts, extent, top_k)
    got = g.voxelPoseSearchScores()
    assert got.dtype == np.int32 and got.shape == want.shape, label
    assert np.array_equal(got, want), f"{label}: {np.argwhere(got != want)[:5].tolist()} got {got[got != want][:5]} want {want[got != want][:5]}"
    wp, ws, wsc = psm.ranking(want, top_k)
    assert len(pose) == min(top_k, want.size), label
    assert np.array_equal(pose, wp) and np.array_equal(shift, ws) and np.array_equal(score, wsc), f"{label}: {pose} {shift.tolist()} {score} vs {wp} {ws.tolist()} {wsc}"
    assert pose.dtype == shift.dtype == score.dtype == np.int32 and cand.dtype == F and cand.shape == (len(pose), 4, 4)
    for i in range(len(pose)):
        assert np.array_equal(cand[i].view(np.uint32), psm.candidate_pose(Ts[pose[i]], shift[i], res).view(np.uint32)), label  # (bits: a pose may hold a NaN)
    return want


def _poses(B):
    Ts = psm.yaw_lattice(np.eye(4), B, 0.6)
    for b in range(B):
        Ts[b, :3, 3] = (0.3 * b, -0.45 * b, 0.2 * b)
    return Ts


# ---- 1. full volumes: every size, pose count, extent and kind of map ----

@pytest.mark.parametrize("kind", ["target", "merged", "rolling"])
@pytest.mark.parametrize("n", [1, 37, 257, 3008])
def test_full_volumes_match_the_model(ng, kind, n):
    g = _kind_engine(ng, kind)
    map_ijk = fm.kind_map(kind).ijk
    assert np.array_equal(np.unique(g.voxelMap()[0], axis=0), np.unique(map_ijk, axis=0))
    src = np.random.default_rng(40 + n).uniform(-4.5, 5.5, (n, 3)).astype(F)
    g.setInputSource(src)
    total = 0
    for B in (1, 3):
        for extent in EXTENTS:
            total += int(_check(g, _poses(B), src, map_ijk, fm.KIND_RES, extent, label=f"{kind} n={n} B={B} extent={extent}").sum())
    assert total > 0
    if kind == "rolling":
        assert g.voxelMapBuilds() == 0
    g.close()


def test_the_anchor_to_voxel_fitness_and_two_identical_calls(ng):
    g = _kind_engine(ng, "target")
    g.setNeighborSearchMethod(1)
    src = np.random.default_rng(7).uniform(-4.5, 5.5, (3008, 3)).astype(F)
    g.setInputSource(src)
    Ts = _poses(5)
    first = g.voxelPoseSearch(Ts, (3, 2, 1), 64)
    vol = g.voxelPoseSearchScores()
    again = g.voxelPoseSearch(Ts, (3, 2, 1), 64)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)) and np.array_equal(vol, g.voxelPoseSearchScores())
    n_matched = g.voxelFitnessBatch(Ts)[3]
    assert np.array_equal(vol[:, 1, 2, 3], n_matched) and n_matched.sum() > 0  # s = 0 is the window's centre
    g.setNeighborSearchMethod(27)  # the neighbourhood setting is not consulted
    assert all(np.array_equal(a, b) for a, b in zip(first, g.voxelPoseSearch(Ts, (3, 2, 1), 64)))
    assert g.voxelPoseSearchKernelMs() > 0.0
    g.close()


# ---- 2. edge cases ----

def test_every_residue_of_the_window_s_first_bit(ng):
    """a map 200 cells long that starts at no multiple of 64, a source with one point in every cell of its length and beyond both ends:
    the window's first bit takes every residue mod 64, in every data word and in both guards"""
    rng = np.random.default_rng(5)
    xs = np.arange(-37, 163)
    keep = rng.random(len(xs)) < 0.6
    keep[[0, -1]] = True
    map_ijk = np.array([(x, y, z) for x in xs[keep] for y in (0, 2) for z in (-1,)] + [(x, 1, -1) for x in xs[~keep]])
    src = _centres([(x, y, -1) for x in range(-37 - 40, 163 + 40) for y in (0, 1)])
    g = _custom(ng, map_ijk)
    g.setInputSource(src)
    for extent in ((31, 1, 0), (5, 2, 0), (0, 0, 0), (17, 0, 1)):
        _check(g, I4[None], src, map_ijk, 0.5, extent, top_k=64, label=f"residues {extent}")
    g.close()


def test_windows_leave_the_grid_through_each_face(ng):
    block = np.array([(x, y, z) for x in range(10) for y in range(10) for z in range(10)])
    line = np.arange(-5, 15)
    src_cells = [(v, 4, 4) for v in line] + [(4, v, 4) for v in line] + [(4, 4, v) for v in line] + [(-5, -5, -5), (14, 14, 14), (-1, 10, 3)]
    src = _centres(src_cells)
    g = _custom(ng, block)
    g.setInputSource(src)
    want = _check(g, I4[None], src, block, 0.5, (3, 3, 3), top_k=64, label="faces")
    assert want.max() > 0 and want.min() < want.max()
    for face, axis in ((-3, 0), (12, 0), (-3, 1), (12, 1), (-3, 2), (12, 2)):  # a source that lies beyond one face only
        cells = np.full((6, 3), 4)
        cells[:, axis] = face + np.sign(4 - face) * (np.arange(6) // 3)
        one = _centres(cells)
        g.setInputSource(one)
        _check(g, I4[None], one, block, 0.5, (3, 2, 3), label=f"face {face} of axis {axis}")
    g.close()


def test_a_source_wholly_outside_the_map_scores_zero_and_ranks_by_index(ng):
    g = _kind_engine(ng, "rolling")
    src = (np.random.default_rng(8).uniform(-2, 2, (300, 3)) + 500.0).astype(F)
    g.setInputSource(src)
    pose, shift, score, _ = g.voxelPoseSearch(_poses(3), (2, 1, 0), 20)
    assert not g.voxelPoseSearchScores().any() and not score.any()
    assert pose.tolist() == [0] * 15 + [1] * 5
    assert shift[:6].tolist() == [[-2, -1, 0], [-1, -1, 0], [0, -1, 0], [1, -1, 0], [2, -1, 0], [-2, 0, 0]]
    _check(g, _poses(3), src, fm.kind_map("rolling").ijk, fm.KIND_RES, (2, 1, 0), top_k=20, label="outside")
    g.close()


def test_nan_far_and_duplicate_points(ng):
    """A source cloud with a non-finite coordinate is refused when it is set (as for every entry), so a NaN coordinate reaches the
    search through the pose: a NaN or infinite entry makes the transformed points NaN or infinite, and they have no cell.  Finite points
    at or beyond 2^20 cells are accepted as a source and have no cell either."""
    g = _kind_engine(ng, "target")
    map_ijk = fm.kind_map("target").ijk
    res = fm.KIND_RES
    src = np.random.default_rng(9).uniform(-3, 4, (400, 3)).astype(F)
    src[10:20] = src[0:10]                    # duplicates count each time
    src[20] = src[21] = src[22] = src[0]
    src[40, 0] = F(LIM * res)                 # at 2^20 cells: no cell
    src[41, 1] = -F(LIM * res) * F(1.5)       # beyond
    src[42, 2] = F(LIM * res) * F(4.0)
    src[43, 0] = np.nextafter(F(LIM * res), F(0))  # the last float below 2^20 cells: it has one
    _raises(ng, ERR_ARG, g.setInputSource, np.array([[0, np.nan, 0]], dtype=F))
    g.setInputSource(src)
    Ts = _poses(7)
    Ts[1, 0, 3] = np.nan        # every point's x is NaN
    Ts[2, 1, 0] = np.nan        # ... y, through a rotation entry (NaN * 0 is NaN too)
    Ts[3, 2, 2] = np.inf        # z is +-inf, or NaN where the point's z is 0
    Ts[4, 0, 3] = F(LIM * res)  # pushed to 2^20 cells and beyond: only the points with x < 0 keep a cell
    Ts[5, :3, 3] = F(3e38)      # far beyond every cell
    for extent in ((0, 0, 0), (3, 2, 1)):
        want = _check(g, Ts, src, map_ijk, res, extent, label=f"nan/far/dup {extent}")
        assert want[0].any() and want[6].any() and not want[1:4].any() and not want[5].any()
    assert not _check(g, Ts[1:4], src, map_ijk, res, (1, 1, 1), label="no cells").any()  # no point has a cell: the source box is empty
    g.close()


def test_cells_next_to_the_key_range(ng):
    """map cells at +-(2^20 - 1): the shifts that would leave (-2^20, 2^20) count nothing, and nothing is read out of bounds"""
    m = LIM - 1
    corners = [([(m, 0, 0), (m - 1, 0, 0), (m, 1, 0)], [(m - 1, 0, 0), (m, 0, 0), (m, 1, 0)]),        # +x
               ([(-m, 3, 0), (-m, 3, 1)], [(-m, 3, 0), (-m + 1, 2, 1)]),                               # -x
               ([(0, m, -m), (0, m - 2, -m)], [(0, m, -m), (1, m - 1, -m + 1)]),                       # +y and -z
               ([(5, -m, m), (5, -m + 1, m - 1)], [(5, -m, m), (4, -m + 2, m)]),                       # -y and +z
               ([(5, 5, m), (5, 5, -m)], [(5, 5, m), (5, 5, -m), (5, 4, m - 1)])]                      # both ends of z in one grid
    for map_cells, src_cells in corners:
        map_ijk, src = np.array(map_cells), _centres(src_cells)
        ijk, has = psm.cells(I4, src, 0.5)
        assert has.all() and ijk.tolist() == [list(c) for c in src_cells]  # the fixtures sit where they are meant to
        g = _custom(ng, map_ijk)
        g.setInputSource(src)
        for extent in ((2, 0, 0), (3, 2, 1), (1, 3, 2)):
            want = _check(g, I4[None], src, map_ijk, 0.5, extent, top_k=64, label=f"key range {map_cells[0]} {extent}")
            assert np.array_equal(want, psm.naive_volume(I4[None], src, map_ijk, 0.5, extent))  # the range rule spelled out
            assert want.any()
        g.close()


def test_ties_on_a_symmetric_map_and_top_k_beyond_the_entries(ng):
    map_ijk = np.array([(-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    src = _centres([(0, 0, 0), (0, 0, 0)])
    g = _custom(ng, map_ijk)
    g.setInputSource(src)
    Ts = np.stack([I4, I4, I4])
    want = _check(g, Ts, src, map_ijk, 0.5, (1, 1, 1), top_k=64, label="ties")
    assert sorted(want.ravel().tolist())[-18:] == [2] * 18 and want.sum() == 36
    pose, shift, score, _ = g.voxelPoseSearch(Ts, (1, 1, 1), 7)
    assert score.tolist() == [2] * 7 and pose.tolist() == [0] * 6 + [1]
    assert shift.tolist() == [[0, 0, -1], [0, -1, 0], [-1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]]
    pose, shift, score, cand = g.voxelPoseSearch(I4[None], (1, 0, 0), 64)  # 3 entries, 64 asked for
    assert pose.tolist() == [0, 0, 0] and shift.tolist() == [[-1, 0, 0], [1, 0, 0], [0, 0, 0]] and score.tolist() == [2, 2, 0] and len(cand) == 3
    g.close()


@pytest.mark.parametrize("B,extent,n", [(300, (3, 2, 1), 37), (70, (31, 31, 0), 37), (16400, (0, 0, 0), 5)])
def test_the_top_k_over_several_levels_and_launches(ng, B, extent, n):
    """8 level-0 segments merged once; 70 segments merged twice; more poses than one launch takes"""
    g = _kind_engine(ng, "target")
    src = np.random.default_rng(60 + n).uniform(-3, 4, (n, 3)).astype(F)
    g.setInputSource(src)
    rng = np.random.default_rng(B)
    Ts = psm.yaw_lattice(np.eye(4), B, 2 * np.pi / B)
    Ts[:, :3, 3] = rng.uniform(-2, 2, (B, 3)).astype(F)
    _check(g, Ts, src, fm.kind_map("target").ijk, fm.KIND_RES, extent, top_k=64, label=f"B={B} {extent}")
    g.close()


# ---- 3. caps, errors, state ----

def test_caps_and_errors_and_a_refused_call_changes_nothing(ng):
    g = _kind_engine(ng, "rolling")
    src = np.random.default_rng(3).uniform(-3, 4, (257, 3)).astype(F)
    Ts = _poses(2)
    _raises(ng, ERR_STATE, g.voxelPoseSearchScores)              # no search yet
    _raises(ng, ERR_STATE, g.voxelPoseSearch, Ts, (1, 1, 1))     # no source
    g.setInputSource(src)
    first = g.voxelPoseSearch(Ts, (3, 2, 1), 8)
    vol, ms = g.voxelPoseSearchScores(), g.voxelPoseSearchKernelMs()
    stats, allocs = g.voxelRollingStats(), g.stats()["device_allocs"]
    big = np.broadcast_to(I4, (1410, 4, 4))
    for bad in [dict(Ts=Ts, extent=(32, 0, 0)), dict(Ts=Ts, extent=(0, 32, 0)), dict(Ts=Ts, extent=(0, 0, 8)), dict(Ts=Ts, extent=(-1, 0, 0)),
                dict(Ts=Ts, extent=(0, -1, 0)), dict(Ts=Ts, extent=(0, 0, -1)), dict(Ts=Ts, extent=(31, 31, 2)), dict(Ts=Ts, extent=(31, 7, 7)),
                dict(Ts=Ts, extent=(1, 1, 1), top_k=0), dict(Ts=Ts, extent=(1, 1, 1), top_k=65), dict(Ts=Ts, extent=(1, 1, 1), top_k=-3),
                dict(Ts=Ts[:0], extent=(1, 1, 1)), dict(Ts=big, extent=(31, 31, 1))]:
        _raises(ng, ERR_ARG, g.voxelPoseSearch, **bad)
        assert np.array_equal(g.voxelPoseSearchScores(), vol) and g.voxelPoseSearchKernelMs() == ms, bad
    L = g._L
    import ctypes as C
    out = np.zeros(8, np.int32); out3 = np.zeros(24, np.int32); m = C.c_size_t(0)
    tc = np.ascontiguousarray(np.transpose(Ts, (0, 2, 1))).reshape(2, 16)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pf = tc.ctypes.data_as(C.POINTER(C.c_float))
    assert L.ngicp_voxel_pose_search(g._h, 2, None, 1, 1, 1, 8, p(out), p(out3), p(out), C.byref(m)) == ERR_ARG
    assert L.ngicp_voxel_pose_search(g._h, 2, pf, 1, 1, 1, 8, None, p(out3), p(out), C.byref(m)) == ERR_ARG
    assert L.ngicp_voxel_pose_search(g._h, 2, pf, 1, 1, 1, 8, p(out), None, p(out), C.byref(m)) == ERR_ARG
    assert L.ngicp_voxel_pose_search(g._h, 2, pf, 1, 1, 1, 8, p(out), p(out3), None, C.byref(m)) == ERR_ARG
    assert L.ngicp_voxel_pose_search(g._h, 2, pf, 1, 1, 1, 8, p(out), p(out3), p(out), None) == ERR_ARG
    assert L.ngicp_voxel_pose_search(g._h, (1 << 24) + 1, pf, 0, 0, 0, 8, p(out), p(out3), p(out), C.byref(m)) == ERR_ARG
    assert L.ngicp_voxel_pose_search_scores(g._h, None, vol.size) == ERR_ARG
    assert L.ngicp_voxel_pose_search_scores(g._h, p(np.zeros(vol.size, np.int32)), vol.size - 1) == ERR_ARG
    assert L.ngicp_voxel_pose_search_kernel_ms(g._h, None) == ERR_ARG and L.ngicp_voxel_pose_search(None, 2, pf, 1, 1, 1, 8, p(out), p(out3), p(out), C.byref(m)) == ERR_ARG
    assert np.array_equal(g.voxelPoseSearchScores(), vol) and g.voxelPoseSearchKernelMs() == ms
    assert g.voxelRollingStats() == stats and g.stats()["device_allocs"] == allocs
    assert all(np.array_equal(a, b) for a, b in zip(first, g.voxelPoseSearch(Ts, (3, 2, 1), 8)))
    # the volume goes with the map it was computed against: every write to the rolling map retires it
    prod = ng.NanoGICP(); prod.setInputSource(src)
    for change in (lambda: g.insertIntoVoxelMap(prod, I4), lambda: g.evictVoxelMap((0, 0, 0), 3.0, 0), lambda: g.clearVoxelMap()):
        g.voxelPoseSearch(Ts, (1, 0, 0), 1); g.voxelPoseSearchScores()
        change()
        _raises(ng, ERR_STATE, g.voxelPoseSearchScores)
    _raises(ng, ERR_STATE, g.voxelPoseSearch, Ts, (1, 0, 0))     # the rolling map is empty
    g.setVoxelResolution(0)
    _raises(ng, ERR_STATE, g.voxelPoseSearch, Ts, (1, 0, 0))     # the voxelized mode is off
    prod.close(); g.close()


def test_the_volume_goes_with_the_target_s_map(ng):
    g = _kind_engine(ng, "target")
    src = np.random.default_rng(4).uniform(-3, 4, (64, 3)).astype(F)
    g.setInputSource(src)
    g.voxelPoseSearch(I4[None], (1, 1, 0), 3); g.voxelPoseSearchScores()
    builds = g.voxelMapBuilds()
    g.setVoxelResolution(0.7)
    _raises(ng, ERR_STATE, g.voxelPoseSearchScores)
    assert g.voxelMapBuilds() == builds  # asking builds nothing
    g.voxelPoseSearch(I4[None], (1, 1, 0), 3); g.voxelPoseSearchScores()
    assert g.voxelMapBuilds() == builds + 1  # ... the search does, once
    g.setInputTarget(src + F(0.25))
    _raises(ng, ERR_STATE, g.voxelPoseSearchScores)
    g.close()


def test_the_grid_s_byte_cap(ng):
    """a map 2^21 - 1 cells long and 1024 rows wide needs 80 bytes a row more than 256 MiB; with 1023 rows it fits"""
    m = LIM - 1
    corners = lambda rows: np.array([(-m, 0, 0), (m, 0, 0), (-m, rows - 1, 0), (m, rows - 1, 0), (0, 5, 0)])
    src = _centres(corners(1024))
    g = _custom(ng, corners(1024))
    g.setInputSource(src)
    _raises(ng, ERR_ARG, g.voxelPoseSearch, I4[None], (1, 1, 0))
    _raises(ng, ERR_STATE, g.voxelPoseSearchScores)  # it changed nothing: there still is no search
    g.close()
    g = _custom(ng, corners(1023))
    src = _centres(corners(1023))
    g.setInputSource(src)
    _check(g, I4[None], src, corners(1023), 0.5, (1, 1, 0), label="just under the cap")
    g.close()


def test_a_search_leaves_an_alignment_s_results_alone(ng):
    tgt, ct = fm.target()
    src, cs_ = fm.source(700)
    g = ng.NanoGICP()
    g.setVoxelResolution(fm.RES)
    g.setInputSource(src); g.setSourceCovariances(cs_)
    g.setInputTarget(tgt); g.setTargetCovariances(ct)
    T = fm.pose((0.05, -0.03, 0.02), (0.5, -0.4, 0.8))
    Ts = _poses(3)

    def search():
        g.voxelPoseSearch(Ts, (3, 2, 1), 8); g.voxelPoseSearchScores(); g.voxelPoseSearchKernelMs()

    search()  # (the workspace exists from here on)
    g.alignBatchVoxel(np.stack([T, I4]))
    lanes = [g.lm_trace(lane=i).copy() for i in range(2)]

    def outcome():
        return (g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.nr_iterations_, g.converged_, g.lm_trace().copy(), g.voxel_correspondences().copy())

    def state():
        return outcome() + (g.stats(),)

    g.align(T)
    aligned = outcome()
    g.linearize(T.astype(np.float64))
    e0 = g.compute_error(T.astype(np.float64))

    before = state()
    search()
    after = state()
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    for i, tr in enumerate(lanes):
        assert np.array_equal(g.lm_trace(lane=i), tr)
    assert g.compute_error(T.astype(np.float64)) == e0
    g.align(T)  # ... and an alignment after a search is the alignment before it, bit for bit
    for a, b in zip(aligned, outcome()):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    want = g.voxelPoseSearch(Ts, (3, 2, 1), 8)
    g.setRobustKernel(1, 1.5)  # HUBER: nothing is refused because a robust kernel or a prior is set, and neither is consulted
    g.setPosePrior(np.eye(4), np.eye(6) * 1e3)
    assert all(np.array_equal(a, b) for a, b in zip(want, g.voxelPoseSearch(Ts, (3, 2, 1), 8)))
    g.close()


# ---- 4. end to end ----

@pytest.fixture(scope="module")
def world(ng):
    """the rolling map of the 12 drive scans in the frame of place 5, at 0.5 m"""
    g, prod = ng.NanoGICP(), ng.NanoGICP()
    g.setVoxelResolution(pc.RES)
    g.setVoxelRolling(True)
    for s, T in zip(cs.drive_scans(pc.N_PLACES), pc.insert_poses()):
        prod.setInputSource(s)
        g.insertIntoVoxelMap(prod, T)
    prod.close()
    assert np.array_equal(np.unique(g.voxelMap()[0], axis=0), pc.map_cells())
    yield g
    g.close()


@pytest.mark.parametrize("move", pc.MOVES)
def test_a_revisit_s_translation_is_found_and_starts_the_alignment(ng, world, move):
    g = world
    q, T_true = pc.query(move)
    g.setInputSource(q)
    Ts = ng.NanoGICP.yawLattice(np.eye(4), pc.N_YAWS, pc.YAW_STEP)
    assert np.array_equal(Ts, pc.lattice())
    pose, shift, score, cand = g.voxelPoseSearch(Ts, pc.EXTENT, 8)
    wp, ws, wsc = pc.model_top(move)
    assert np.array_equal(g.voxelPoseSearchScores(), pc.model_volume(move))
    assert np.array_equal(pose, wp) and np.array_equal(shift, ws) and np.array_equal(score, wsc)
    assert 5 * int(pose[0]) == 35 and shift[0].tolist() == [round(move[0] / pc.RES), round(move[1] / pc.RES), 0]
    print(f"move {move}: top {score[:3].tolist()} at {[5 * int(p) for p in pose[:3]]} deg {shift[:3].tolist()}, kernels {g.voxelPoseSearchKernelMs():.3f} ms")
    # exact GICP against the scan of place 5, from the candidate and from the truth
    e = ng.NanoGICP()
    e.setInputSource(q); e.setInputTarget(cs.drive_scans(pc.N_PLACES)[pc.PLACE])
    e.align(cand[0])
    T_ps, ok_ps = e.getFinalTransformation().copy(), e.hasConverged()
    e.align(T_true.astype(F))
    T_gt, ok_gt = e.getFinalTransformation().copy(), e.hasConverged()
    dt, dr = clouds.pose_error(T_ps, T_gt)
    print(f"exact align from the candidate vs from the truth: {dt:.2e} m, {dr:.2e} rad")
    assert ok_ps and ok_gt
    assert dt <= 2.0 * e._p["trans_eps"] and dr <= 2.0 * e._p["rot_eps"]
    e.close()
    # a report, nothing asserted: where a voxelized DIRECT1 align on the rolling map ends from the yaw-only guess and from the candidate
    for name, guess in (("the yaw-only guess", Ts[pose[0]]), ("the candidate", cand[0])):
        g.align(guess)
        dt, dr = clouds.pose_error(g.getFinalTransformation(), T_true)
        print(f"voxelized DIRECT1 align on the rolling map from {name}: converged {g.hasConverged()}, {dt:.3f} m and {dr:.4f} rad from the truth")


def test_the_shim_agrees_with_python(ng, tmp_path):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(tmp_path), "pose_search_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_search_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    scans = cs.drive_scans(12)[4:7]
    q, _ = cs.revisit(5, 12, move=(1.2, -0.8, 0.0))
    Ts = ng.NanoGICP.yawLattice(np.eye(4), 12, np.radians(30.0))
    paths = []
    for name, c in [("query", q)] + [(f"kf{i}", s) for i, s in enumerate(scans)]:
        paths.append(os.path.join(str(tmp_path), name + ".bin"))
        np.ascontiguousarray(c, dtype=F).tofile(paths[-1])
    poses = os.path.join(str(tmp_path), "poses.bin")
    np.ascontiguousarray(np.transpose(Ts, (0, 2, 1))).tofile(poses)
    run = subprocess.run([exe, "0.5", "6", "5", "1", "5", poses] + paths, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines()]
    one = {ln[0]: ln[1:] for ln in lines if ln[0] != "cand"}
    g, prod = ng.NanoGICP(), ng.NanoGICP()
    g.setVoxelResolution(0.5); g.setVoxelRolling(True)
    for s in scans:
        prod.setInputSource(s); g.insertIntoVoxelMap(prod, I4)
    g.setInputSource(q)
    pose, shift, score, cand = g.voxelPoseSearch(Ts, (6, 5, 1), 5)
    vol = g.voxelPoseSearchScores().ravel().astype(np.int64)
    assert one["empty_map"] == ["0"] and "rolling voxel map is empty" in run.stderr
    assert one["voxels"] == [str(g.getVoxelMapSize())] and one["no_search"] == ["0"] and one["found"] == ["5"]
    got = [ln[1:] for ln in lines if ln[0] == "cand"]
    assert len(got) == 5
    for i, tok in enumerate(got):
        assert [int(t) for t in tok[:5]] == [pose[i], *shift[i], score[i]]
        assert np.array_equal(np.array([float.fromhex(t) for t in tok[5:]], dtype=F).reshape(4, 4).T, cand[i])
    assert one["volume"] == [str(vol.size), str(vol.sum()), str(int((np.arange(vol.size) % 9973 * vol).sum()))]
    assert one["bad_extent"] == ["0"] and one["kept"] == [str(vol.size)] and one["timed"] == ["1"]
    assert one["lattice"][0] == "4" and float.fromhex(one["lattice"][1]) == 1.0 and float.fromhex(one["lattice"][2]) == -1.0
    prod.close(); g.close()
