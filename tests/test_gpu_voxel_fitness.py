"""The voxel fitness on the GPU (ngicp_voxel_fitness / _batch / _points; k_voxel_fitness<K> and k_voxel_fitness_final in
csrc/ngicp_voxel_fitness.h) against the numpy model of its definition (tests/_voxel_fitness_model.py, which proves itself - and the
fixtures used here - in test_voxel_fitness_model_cpu.py).

Tolerances: counts and per-point voxel numbers exact; per-point m / sqd and the per-pose means within 1e-9 relative, what this project
holds the same terms to (tests/test_gpu_vgicp_rolling.py, the hooks' H / b / err); bit-equality of the per-point values is expected and
printed.  Batch lanes, repeated calls and the shim are compared bit for bit.  No point is exempted anywhere: the CPU tests show that on
these fixtures no gate and no runner-up slot is closer than 1e-6 relative to a value it could be confused with."""
import os
import subprocess

import numpy as np
import pytest

import _batch_cases as bc
import _vgicp_batch_cases as vbc
import _vgicp_model as vm
import _voxel_fitness_model as fm
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -2, -3
DBL_MAX = fm.DBL_MAX
I4 = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture(scope="module")
def tgt():
    pts, covs = fm.target()
    return {"pts": pts, "covs": covs, "map": vm.VoxelMap(pts, covs, fm.RES)}


def _engine(ng, src, cs, tgt, K, res=fm.RES):
    g = ng.NanoGICP()
    g.setVoxelResolution(res)
    g.setNeighborSearchMethod(K)
    g.setInputSource(src); g.setSourceCovariances(cs)
    g.setInputTarget(tgt["pts"]); g.setTargetCovariances(tgt["covs"])
    return g


def _raises(ng, code, fn, *a):
    with pytest.raises(ng.NgicpError) as e:
        fn(*a)
    assert e.value.code == code, f"{e.value}"


def _close(got, want, label):
    """within 1e-9 relative, entry by entry; infinities and the -1 of an unmatched point exactly; -> bit-equal"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, label
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), label
    off = np.abs(got[fin] - want[fin])
    assert (off <= 1e-9 * np.abs(want[fin])).all(), f"{label}: off by {(off / np.maximum(np.abs(want[fin]), 1e-300)).max():.2e} relative"
    return np.array_equal(got, want)


def _check_pose(g, model_map, src, cs, T, K, label):
    """the per-point values and, under every gate of the fixtures, the record of the pose T against the model's"""
    m, d, v, matched, _ = fm.point_values(src, cs, model_map, T, K)
    gm, gd, gv = g.voxel_fitness_points(T)
    assert gv.dtype == np.int32 and np.array_equal(gv, v), f"{label}: voxel numbers differ at {np.flatnonzero(gv != v)[:5].tolist()}"
    assert np.array_equal(gm == -1, ~matched) and np.array_equal(gd[~matched], np.full((~matched).sum(), -1.0)), f"{label}: unmatched points"
    bits = _close(gm, m, label + " m") & _close(gd, d, label + " sqd")
    for gate in fm.GATES:
        want = fm.score(src, cs, model_map, T, K, gate)
        got = g.voxelFitness(gate, T)
        assert (got["n_matched"], got["n_inliers"]) == (want["n_matched"], want["n_inliers"]), f"{label}, gate {gate}: {got} vs {want}"
        for key in ("mahalanobis", "sqdist"):
            if want["n_inliers"] == 0:
                assert got[key] == DBL_MAX, f"{label}, gate {gate}"
            else:
                assert abs(got[key] - want[key]) <= 1e-9 * abs(want[key]), f"{label}, gate {gate}: {key} {got[key]!r} vs {want[key]!r}"
    return bits, int(matched.sum())


# ---- 1. against the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", fm.NEIGHBORS)
@pytest.mark.parametrize("n", fm.SIZES)
def test_points_and_scores_match_the_model(ng, tgt, n, K):
    """1 .. 700 source points (the wave and block edges of a 256-thread block) with random SPD covariances against the map of a random
    cube plus lattice-plane points, at three poses and four gates."""
    src, cs = fm.source(n)
    g = _engine(ng, src, cs, tgt, K)
    for name, T in fm.POSES.items():
        bits, matched = _check_pose(g, tgt["map"], src, cs, T, K, f"{n} points, DIRECT{K}, {name}")
        print(f"{n} points, DIRECT{K}, {name}: {matched} matched, per-point values bit-equal: {bits}")
    assert g.voxelMapBuilds() == 1
    g.close()


# ---- 2. every kind of map ------------------------------------------------------------------------------------------------------------------
def _kind_engine(ng, kind, K):
    (a, ca), (b, cb) = fm.kind_clouds()
    g, prod = ng.NanoGICP(), ng.NanoGICP()
    g.setVoxelResolution(fm.KIND_RES)
    g.setNeighborSearchMethod(K)
    if kind == "target":
        g.setInputTarget(np.r_[a, b]); g.setTargetCovariances(np.r_[ca, cb])
    elif kind == "merged":
        g.setVoxelSubmapMerge(True)
        for p, c in ((a, ca), (b, cb)):
            prod.setInputSource(p); prod.setSourceCovariances(c)
            g.addKeyframe(prod)
        g.setSubmapKeyframes([0, 1])
    else:  # no target is ever set on this handle
        g.setVoxelRolling(True)
        for (p, c), T in zip(((a, ca), (b, cb)), fm.ROLL_POSES):
            prod.setInputSource(p); prod.setSourceCovariances(c)
            g.insertIntoVoxelMap(prod, T)
        assert g.evictVoxelMap(fm.ROLL_EVICT[0], fm.ROLL_EVICT[1], 0) > 0
    prod.close()
    return g


@pytest.mark.parametrize("kind", ["target", "merged", "rolling"])
def test_every_kind_of_map(ng, kind):
    """the target-built map, the one merged from two keyframes' voxel sums, and the rolling one after two inserts and an eviction, with no
    target ever set on that handle - the case no other score of the engine serves"""
    model_map = fm.kind_map(kind)
    src, cs = fm.kind_source()
    for K in fm.NEIGHBORS:
        g = _kind_engine(ng, kind, K)
        g.setInputSource(src); g.setSourceCovariances(cs)
        assert g.getVoxelMapSize() == len(model_map)
        for name, T in fm.POSES.items():
            bits, matched = _check_pose(g, model_map, src, cs, T, K, f"{kind} map, DIRECT{K}, {name}")
            print(f"{kind} map ({len(model_map)} voxels), DIRECT{K}, {name}: {matched} of {len(src)} matched, bit-equal: {bits}")
        if kind == "merged":
            assert g.voxelMapMergeStats()["merged_builds"] == 1
        if kind == "rolling":
            assert g.voxelMapBuilds() == 0
            _raises(ng, ERR_STATE, g.fitness)  # the exact score has no target to search
        g.close()


# ---- 3. batch equals single ------------------------------------------------------------------------------------------------------------------
def _single(g, T, gate):
    f = g.voxelFitness(gate, T)
    return f["mahalanobis"], f["sqdist"], f["n_inliers"], f["n_matched"]


def _lane(batch, i):
    return tuple(x[i].item() for x in batch)


@pytest.mark.parametrize("K", fm.NEIGHBORS)
def test_a_batch_lane_is_the_single_call_bit_for_bit(ng, tgt, K):
    src, cs = fm.source(700)
    g = _engine(ng, src, cs, tgt, K)
    Ts = np.stack(list(fm.POSES.values()))
    for gate in (2.5, DBL_MAX):
        for B in (1, 3):
            batch = g.voxelFitnessBatch(Ts[:B], gate)
            assert [x.dtype for x in batch] == [np.float64, np.float64, np.int64, np.int64] and all(x.shape == (B,) for x in batch)
            for i in range(B):
                assert _lane(batch, i) == _single(g, Ts[i], gate), f"DIRECT{K}, gate {gate}, B {B}, lane {i}"
            again = g.voxelFitnessBatch(Ts[:B], gate)
            assert all(np.array_equal(x, y) for x, y in zip(batch, again))
    assert g.voxelMapBuilds() == 1
    g.close()


def test_a_batch_that_crosses_the_launch_s_chunk(ng, tgt):
    """4097 distinct poses of a 65-point source under DIRECT1: the last lane of the first launch, the first and last of the second"""
    src, cs = fm.source(65)
    g = _engine(ng, src, cs, tgt, 1)
    B = 4097
    Ts = np.stack([fm.pose((0.0005 * i, -0.0003 * i, 0.0002 * i), (0.0, 0.0, 0.01 * i)) for i in range(B)])
    batch = g.voxelFitnessBatch(Ts, 40.0)
    for i in (0, 4095, 4096, B - 1):
        assert _lane(batch, i) == _single(g, Ts[i], 40.0), f"lane {i}"
    assert len({_lane(batch, i) for i in (0, 4095, 4096)}) == 3  # distinct poses, distinct records
    again = g.voxelFitnessBatch(Ts, 40.0)
    assert all(np.array_equal(x, y) for x, y in zip(batch, again))
    g.close()


# ---- 4. the handle is left alone ------------------------------------------------------------------------------------------------------------
def test_scoring_leaves_the_handle_alone(ng, tgt):
    src, cs = fm.source(700)
    g = _engine(ng, src, cs, tgt, 7)
    Ts = np.stack(list(fm.POSES.values()))
    G = np.stack([fm.POSES["small"], I4])
    g.voxelFitnessBatch(Ts, 2.5); g.voxel_fitness_points(I4)  # (the query's workspace exists from here on: stats()["device_allocs"] stays)
    g.alignBatchVoxel(G)
    lanes = [g.lm_trace(lane=i).copy() for i in range(len(G))]
    g.align(fm.POSES["small"])
    before = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), g.nr_iterations_, g.converged_, g.voxel_correspondences().copy(),
              g.correspondences(), g.stats(), g.voxelMapBuilds())

    def after():
        return (g.getFinalTransformation(), g.lm_trace(), g.getFinalHessian(), g.nr_iterations_, g.converged_, g.voxel_correspondences(), g.correspondences(), g.stats(),
                g.voxelMapBuilds())

    def same(a, b):
        for k, (x, y) in enumerate(zip(a, b)):
            if isinstance(x, dict):
                assert x == y, {key: (x[key], y[key]) for key in x if x[key] != y[key]}
            elif isinstance(x, tuple):
                assert all(np.array_equal(p, q) for p, q in zip(x, y)), k
            else:
                assert np.array_equal(np.asarray(x), np.asarray(y)), k

    g.voxelFitnessBatch(Ts, 2.5)
    g.voxelFitness()
    g.voxel_fitness_points()
    same(before, after())
    for i, tr in enumerate(lanes):
        assert np.array_equal(g.lm_trace(lane=i), tr), f"lane {i} of the earlier alignBatchVoxel"
    # the state compute_error evaluates, frozen by a linearize
    T1 = fm.pose((0.3, 0.1, 0.02), (0.5, -0.3, 2.0)).astype(np.float64)
    T2 = fm.pose((0.31, 0.09, 0.02), (0.5, -0.3, 2.0)).astype(np.float64)
    g.linearize(T1)
    e, cn = g.compute_error(T2), g.voxel_correspondences().copy()
    g.voxelFitnessBatch(Ts, 40.0)
    assert g.compute_error(T2) == e and np.array_equal(g.voxel_correspondences(), cn)
    # a fresh map is not rebuilt; a stale one is built once by a call, however many poses it scores
    builds = g.voxelMapBuilds()
    g.voxelFitnessBatch(Ts)
    assert g.voxelMapBuilds() == builds
    g.setInputTarget(tgt["pts"][100:700].copy()); g.setTargetCovariances(tgt["covs"][100:700].copy())
    g.voxelFitnessBatch(Ts)
    assert g.voxelMapBuilds() == builds + 1
    g.voxelFitness(); g.voxel_fitness_points()
    assert g.voxelMapBuilds() == builds + 1
    g.close()


# ---- 5. edges and errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(ng, tgt):
    import ctypes as C
    src, cs = fm.source(257)
    L = ng.load_library()
    g = _engine(ng, src, cs, tgt, 7)
    one, out = np.ascontiguousarray(I4.T.reshape(16)), ng.VoxelFitness()
    f32, f64, i32 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    p = lambda a, ty: a.ctypes.data_as(ty)
    m, d, v = np.empty(257), np.empty(257), np.empty(257, np.int32)
    # the voxel mode off
    g.setVoxelResolution(0)
    _raises(ng, ERR_STATE, g.voxelFitness)
    _raises(ng, ERR_STATE, g.voxelFitnessBatch, I4[None])
    _raises(ng, ERR_STATE, g.voxel_fitness_points)
    g.setVoxelResolution(fm.RES)
    # n == 0, null pointers, a short capacity, a bad gate
    _raises(ng, ERR_ARG, g.voxelFitnessBatch, np.zeros((0, 4, 4), np.float32))
    assert L.ngicp_voxel_fitness(g._h, p(one, f32), 1.0, None) == ERR_ARG
    assert L.ngicp_voxel_fitness_batch(g._h, 1, None, 1.0, C.byref(out)) == ERR_ARG
    assert L.ngicp_voxel_fitness_batch(g._h, 1, p(one, f32), 1.0, None) == ERR_ARG
    for args in ((None, p(d, f64), p(v, i32)), (p(m, f64), None, p(v, i32)), (p(m, f64), p(d, f64), None)):
        assert L.ngicp_voxel_fitness_points(g._h, p(one, f32), *args, 257) == ERR_ARG
    assert L.ngicp_voxel_fitness_points(g._h, p(one, f32), p(m, f64), p(d, f64), p(v, i32), 256) == ERR_ARG
    assert L.ngicp_voxel_fitness_points(g._h, p(one, f32), p(m, f64), p(d, f64), p(v, i32), 257) == 0
    for gate in (float("nan"), -1.0, -0.0 - 1e-300, float("-inf")):
        _raises(ng, ERR_ARG, g.voxelFitness, gate)
        _raises(ng, ERR_ARG, g.voxelFitnessBatch, I4[None], gate)
    assert g.voxelMapBuilds() == 1  # (only the one valid call built anything)
    g.close()
    # no source: as align; an empty rolling map
    h = ng.NanoGICP()
    h.setVoxelResolution(fm.RES)
    h.setInputTarget(tgt["pts"])
    _raises(ng, ERR_STATE, h.voxelFitness)
    _raises(ng, ERR_STATE, h.voxel_fitness_points, I4)
    h.setInputSource(src)
    h.setVoxelRolling(True)
    _raises(ng, ERR_STATE, h.voxelFitness)
    _raises(ng, ERR_STATE, h.voxelFitnessBatch, I4[None])
    h.close()


def test_edges(ng, tgt):
    src, cs = fm.source(257)
    for K in fm.NEIGHBORS:
        g = _engine(ng, src, cs, tgt, K)
        # every point out of range: no cell, beyond 2^20 voxels, a NaN pose
        bad = np.full((4, 4), np.nan, np.float32)
        for T in (fm.pose((2.0 ** 20 * fm.RES, 0.0, 0.0)), fm.pose((0.0, -3e9, 0.0)), bad):
            assert g.voxelFitness(DBL_MAX, T) == {"mahalanobis": DBL_MAX, "sqdist": DBL_MAX, "n_inliers": 0, "n_matched": 0}
            m, d, v = g.voxel_fitness_points(T)
            assert (m == -1).all() and (d == -1).all() and (v == -1).all()
        # at the range's +x edge (cells up to 2^20 - 1: the centre in range, its +x neighbour not; beyond it no cell): nothing is occupied
        assert g.voxelFitness(DBL_MAX, fm.pose(((2.0 ** 20 - 6) * fm.RES, 0.0, 0.0)))["n_matched"] == 0
        # a gate of 0 keeps the points whose term is exactly 0 - none here - and counts the matched ones all the same
        f0, f = g.voxelFitness(0.0, I4), g.voxelFitness(DBL_MAX, I4)
        assert f0["n_inliers"] == 0 and f0["mahalanobis"] == DBL_MAX and f0["n_matched"] == f["n_matched"] == f["n_inliers"] > 0
        # the robust kernel, the pose prior and max_correspondence_distance are not consulted
        Ts = np.stack(list(fm.POSES.values()))
        plain, pts = g.voxelFitnessBatch(Ts, 2.5), g.voxel_fitness_points(Ts[1])
        g.setRobustKernel(ng.RobustKernel.CAUCHY, 0.5)
        g.setPosePrior(np.eye(4), np.eye(6) * 1e3)
        g.setMaxCorrespondenceDistance(1e-3)
        assert all(np.array_equal(x, y) for x, y in zip(plain, g.voxelFitnessBatch(Ts, 2.5)))
        assert all(np.array_equal(x, y) for x, y in zip(pts, g.voxel_fitness_points(Ts[1])))
        g.close()
    # the source's covariances are computed if missing, exactly as align does
    a, b = ng.NanoGICP(), ng.NanoGICP()
    for e in (a, b):
        e.setVoxelResolution(fm.RES)
        e.setInputSource(tgt["pts"][:500]); e.setInputTarget(tgt["pts"]); e.setTargetCovariances(tgt["covs"])
    a.calculateSourceCovariances()
    assert a.voxelFitness(DBL_MAX, I4) == b.voxelFitness(DBL_MAX, I4)
    assert np.array_equal(a.getSourceCovariances(), b.getSourceCovariances())
    a.close(); b.close()


# ---- 6. ranking candidate poses in a restored rolling map ------------------------------------------------------------------------------------
def test_the_engine_ranks_the_lanes_as_the_model_does(ng):
    """INTEGRATION.md's relocalisation recipe on the twelve guesses of tests/_batch_cases.py with the settings of
    tests/_vgicp_batch_cases.py: the 60k map is a rolling map saved in one handle and restored in another that never sees a target;
    alignBatchVoxel, then voxelFitnessBatch.  Asserted: every lane's counts equal the model's, its scores within 1e-9, and the engine's
    ordering of the lanes by score is the model's.  What the ordering shows is printed and recorded in DESIGN.md 4.18; nothing is asserted
    about how well the score separates the minima."""
    w = bc.workload()
    G = bc.guesses(w)
    mapper, g = ng.NanoGICP(), ng.NanoGICP()
    for e in (mapper, g):
        e.setVoxelResolution(vbc.RES)
        e.setVoxelRolling(True)
    mapper.setInputSource(w.target)
    mapper.insertIntoVoxelMap(mapper, I4)
    saved, inserts = mapper.rollingVoxelMap(), mapper.voxelRollingStats()["inserts"]
    mapper.close()
    vbc.configure(g)
    g.setRollingVoxelMap(*saved, inserts)
    g.setInputSource(w.source)
    T, conv, its, _ = g.alignBatchVoxel(G)
    got = g.voxelFitnessBatch(T)
    cs = g.getSourceCovariances()
    model_map = fm.RecordMap(vbc.RES, saved[0], saved[1], saved[2], saved[3])
    want = [fm.score(w.source, cs, model_map, t, vbc.NEIGHBORS) for t in T]
    n = len(w.source)
    for i, s in enumerate(want):
        e = clouds.pose_error(T[i], T[0])
        print(f"lane {i}: {int(its[i]) + 1} iterations, converged {bool(conv[i])}, {e[0]:.2e} m / {e[1]:.2e} rad from lane 0; mahalanobis {got[0][i]:.6g} "
              f"(model {s['mahalanobis']:.6g}), sqdist {got[1][i]:.6g}, overlap {got[3][i] / n:.4f}")
        assert (int(got[2][i]), int(got[3][i])) == (s["n_inliers"], s["n_matched"]), f"lane {i}"
        for k, key in enumerate(("mahalanobis", "sqdist")):
            assert abs(got[k][i] - s[key]) <= 1e-9 * abs(s[key]), f"lane {i}: {key} {got[k][i]!r} vs {s[key]!r}"
    order = np.argsort(got[0], kind="stable")
    assert np.array_equal(order, np.argsort([s["mahalanobis"] for s in want], kind="stable"))
    print("lanes by score:", order.tolist())
    g.close()


# ---- 7. the C++ shim -------------------------------------------------------------------------------------------------------------------------
def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "voxel_fitness_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "voxel_fitness_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_shim_gives_the_python_api_s_bytes(ng, tmp_path):
    sc = clouds.make_scene()
    scans = [clouds.vlp16(sc, clouds.make_pose((0.3 * i, 0.1 * i, 0.0)), 400 + i, cols=188) for i in range(2)]
    res, gate = 1.0, 12.5
    paths = []
    for i, a in enumerate(scans):
        p = tmp_path / f"scan{i}.bin"
        np.ascontiguousarray(a[:, :3], np.float32).tofile(p)
        paths.append(str(p))
    exe = _build(tmp_path)
    out = subprocess.run([exe, repr(res), repr(gate), str(tmp_path / "points.bin"), *paths], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    rows = {l[0]: l[1:] for l in lines}
    rec = lambda l: (int(l[0]), float.fromhex(l[1]), float.fromhex(l[2]), int(l[3]), int(l[4]))
    assert rec(rows["mode_off"])[0] == 0 and rec(rows["empty_map"])[0] == 0

    mapper, g = ng.NanoGICP(), ng.NanoGICP()
    for e in (mapper, g):
        e.setVoxelResolution(res)
        e.setVoxelRolling(True)
    mapper.setInputSource(scans[0])
    n_new, _ = mapper.insertIntoVoxelMap(mapper, I4)
    assert rows["insert"] == ["1", str(n_new)]
    g.setInputSource(scans[1])
    g.setRollingVoxelMap(*mapper.rollingVoxelMap(), mapper.voxelRollingStats()["inserts"])
    assert rows["restored"] == ["1"]
    shifted = lambda x, y: fm.pose((x, y, 0.0))
    G = np.stack([I4, shifted(0.3, -0.2), shifted(25.0, 0.0)])
    finals = g.alignBatchVoxel(G)[0]
    assert rows["lanes"] == ["3"]
    scores = g.voxelFitnessBatch(finals, gate)
    best = 0
    for i, l in enumerate(l[1:] for l in lines if l[0] == "lane"):
        assert rec(l) == (1,) + _lane(scores, i), f"lane {i}"
        if 2 * scores[3][i] >= len(scans[1]) and scores[0][i] < scores[0][best]:
            best = i
    assert rows["best"] == [str(best)]
    g.align(G[best])
    f = g.voxelFitness(gate)
    assert rec(rows["final"]) == (1, f["mahalanobis"], f["sqdist"], f["n_inliers"], f["n_matched"])
    f = g.voxelFitness()
    assert rec(rows["final_ungated"]) == (1, f["mahalanobis"], f["sqdist"], f["n_inliers"], f["n_matched"]) and f["n_matched"] > 0
    m, d, v = g.voxel_fitness_points(finals[best])
    n = len(scans[1])
    assert rows["points"] == ["1", str(n)]
    raw = open(tmp_path / "points.bin", "rb").read()
    assert raw == m.tobytes() + d.tobytes() + v.tobytes()
    assert (v >= 0).any() and (v == -1).any()
    mapper.close(); g.close()
