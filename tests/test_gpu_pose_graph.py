"""The pose graph on the GPU (ngicp_pose_graph_*; csrc/ngicp_pose_graph.h) against the numpy model of the definition
(tests/_pose_graph_model.py, which proves itself in test_pose_graph_model_cpu.py).  The graphs are the smallest that cross each boundary
(tests/_pose_graph_cases.py): 2 nodes; 3 with the middle one fixed; chains of 65 and 257 (one more than a wave, than a block); a ring of
24 with one loop edge; a star whose hub has 130 edges; multi-edges and reversed edges; two components; a chain of 4097 with 40 loop edges.

Tolerances.  Double-valued results (residuals, s, w, chi2, gradient, blocks, products): 1e-9 of the largest magnitude of the compared
array, the project's tolerance for such results.  Optimised poses: ten times the largest difference between the model with its direct
solve and the model with its own conjugate gradients (pc.MEASURED_CG_DIFF, measured on the CPU by test_pose_graph_model_cpu.py): 3e-11 on
every fixture but big4097, 7e-8 on big4097, which stops after two outer iterations and runs at cg_tol = 1e-11 (pc.CASE_OPTIONS says why)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _keyframe_move_model as km
import _pose_graph_cases as pc
import _pose_graph_model as pgm
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu
ERR_ARG = -2


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _load(ng, g):
    e = ng.NanoGICP()
    assert e.poseGraphAddNodes(g.poses, g.fixed) == 0
    assert e.poseGraphAddEdges(g.ij, g.Z, g.info, g.flags) == 0
    e.poseGraphSetRobust(g.kind, g.width)
    return e


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-300)
    err = float(np.abs(got - want).max()) / scale if want.size else 0.0
    print(f"  {what}: {err:.2e} of {scale:.3g}")
    assert got.shape == want.shape and err <= 1e-9, (what, err)


@functools.lru_cache(maxsize=None)
def _model_run(name):
    """the model with its direct solve on a fixture, once: (start graph, result, final poses, truth)"""
    g, truth = pc.CASES[name]()
    start = g.copy()
    opt = pc.options(name)
    res = pgm.optimize(g, "direct", **opt)
    pc.assert_margins(res, opt)  # on the model alone, before the engine is looked at: no gain ratio within 1e-6 of the threshold
    return start, res, g.poses, truth


def _pose_tolerance(name):
    return 10.0 * pc.MEASURED_CG_DIFF[name if name in pc.MEASURED_CG_DIFF else "default"]


# ---------------------------------------------------------------------------------------------------------------- 1. linearize
@pytest.mark.parametrize("kind", [pgm.NONE, pgm.HUBER, pgm.CAUCHY, pgm.GEMAN_MCCLURE])
@pytest.mark.parametrize("name", list(pc.CASES))
def test_linearize_matches_the_model(ng, name, kind):
    g, _ = pc.CASES[name]()
    g.flags = np.arange(g.m) % 2 == 1  # every other edge is flagged
    s0 = pgm.linearize(g).s
    g.kind, g.width = kind, float(np.sqrt(np.median(s0)))  # a width with terms on both sides of it
    e = _load(ng, g)
    got, want = e.poseGraphLinearize(), pgm.linearize(g)
    if kind != pgm.NONE and g.m > 3:
        assert (want.w[g.flags] < 1.0).any() and (want.w[~g.flags] == 1.0).all()
    _close(got["r"], want.r, "r")
    _close(got["s"], want.s, "s")
    _close(got["w"], want.w, "w")
    _close([got["chi2"]], [want.chi2], "chi2")
    _close(got["grad"], want.grad, "gradient")
    _close(got["diag"], want.diag, "diagonal blocks")
    assert not got["grad"][g.fixed].any() and not got["diag"][g.fixed].any()  # fixed nodes: zero, as the header says
    assert np.array_equal(e.poseGraphPoses(), g.poses)                          # the hook leaves the poses alone


# ---------------------------------------------------------------------------------------------------------------- 2. multiply
@pytest.mark.parametrize("name", list(pc.CASES))
def test_multiply_matches_the_model_s_matrix(ng, name):
    g, _ = pc.CASES[name]()
    e = _load(ng, g)
    L = pgm.linearize(g)
    x = np.random.default_rng(7).normal(size=(g.n, 6))
    for lam in (0.0, 1e-3 * float(np.abs(np.einsum("nii->ni", L.diag)).max())):
        y = e.poseGraphMultiply(lam, x)
        _close(y, pgm.multiply(L, lam, x), f"(H + {lam:.3g} I) x")
        assert not y[g.fixed].any()


# ---------------------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("name", ["star130", "chain257", "two_components"])
def test_two_runs_on_fresh_handles_are_bit_equal(ng, name):
    g, _ = pc.CASES[name]()
    out = []
    for _ in range(2):
        e = _load(ng, g)
        res = e.poseGraphOptimize(**pc.options(name))
        out.append((e.poseGraphPoses(), res))
    (pa, ra), (pb, rb) = out
    assert np.array_equal(pa, pb) and np.array_equal(ra["trace"], rb["trace"])
    for k in ("initial_chi2", "final_chi2", "iterations", "accepted", "cg_iterations", "converged"):
        assert ra[k] == rb[k], k
    assert ra["accepted"] >= 2 and ra["cg_iterations"] > 10


# ---------------------------------------------------------------------------------------------------------------- 4. optimize
def _compare_with_model(ng, name):
    start, want, want_poses, truth = _model_run(name)
    e = _load(ng, start)
    opt = pc.options(name)
    got = e.poseGraphOptimize(**opt)
    poses = e.poseGraphPoses()
    diff = pc.pose_difference(poses, want_poses)
    print(f"  {name}: pose difference to the model {diff:.3g} (tolerance {_pose_tolerance(name):.3g}); tries {len(got['trace'])}, "
          f"cg iterations {got['cg_iterations']}, chi2 {got['initial_chi2']:.6g} -> {got['final_chi2']:.6g}, kernel {e.poseGraphKernelMs():.1f} ms; "
          f"distance from the ground truth {pc.pose_difference(poses, truth):.3g}")
    assert [int(t[4]) for t in got["trace"]] == [t[4] for t in want["trace"]]  # the accept / reject sequence
    assert got["iterations"] == want["iterations"] and got["accepted"] == want["accepted"] and got["converged"] == want["converged"]
    assert diff <= _pose_tolerance(name)
    assert np.array_equal(poses[start.fixed], start.poses[start.fixed])
    _close([got["initial_chi2"]], [want["initial_chi2"]], "initial chi2")
    if want["final_chi2"] > 1e-12 * want["initial_chi2"]:  # below that the final chi2 is the residuals' own rounding: "zero"
        _close([got["final_chi2"]], [want["final_chi2"]], "final chi2")
    else:
        assert got["final_chi2"] <= 1e-12 * want["initial_chi2"]
    assert (got["trace"][:, 3] <= opt["cg_max_iterations"]).all() and got["cg_iterations"] == int(got["trace"][:, 3].sum())
    return poses, truth


@pytest.mark.parametrize("name", [n for n in pc.CASES if not n.startswith("false_edge")])  # (those two: check 5 below)
def test_optimize_matches_the_model_with_the_direct_solve(ng, name):
    _compare_with_model(ng, name)


# ---------------------------------------------------------------------------------------------------------------- 5. robust edges
@pytest.mark.parametrize("name", ["false_edge_none", "false_edge_cauchy"])
def test_a_false_loop_edge_under_none_and_under_cauchy(ng, name):
    """The engine matches the model as in check 4 (the NONE run is the one with rejected tries in its trace).  Recorded, not
    asserted against a number chosen in advance: the distance of each result from the ground truth."""
    poses, truth = _compare_with_model(ng, name)
    print(f"  {name}: distance from the ground truth {pc.pose_difference(poses, truth):.3g}")


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def _snapshot(e):
    return e.poseGraphSize(), e.poseGraphPoses(), e.poseGraphEdges(), e.poseGraphFixed()


def _same_graph(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and np.array_equal(a[3], b[3])


def test_refused_calls_change_nothing(ng):
    g, _ = pc.ring24()
    e = _load(ng, g)
    keep = _snapshot(e)
    eye, info = np.eye(4)[None], np.eye(6)[None]
    nan_Z = eye.copy()
    nan_Z[0, 1, 2] = np.nan
    asym = info.copy()
    asym[0, 2, 4] = 1e-300
    bad_row = eye.copy()
    bad_row[0, 3, 1] = 1e-9
    calls = {
        "a self-edge": lambda: e.poseGraphAddEdges([[3, 3]], eye, info),
        "an unknown id": lambda: e.poseGraphAddEdges([[0, 24]], eye, info),
        "a negative id": lambda: e.poseGraphAddEdges([[-1, 2]], eye, info),
        "a NaN in Z": lambda: e.poseGraphAddEdges([[0, 1]], nan_Z, info),
        "a last row": lambda: e.poseGraphAddEdges([[0, 1]], bad_row, info),
        "an asymmetric information": lambda: e.poseGraphAddEdges([[0, 1]], eye, asym),
        "all or nothing": lambda: e.poseGraphAddEdges([[0, 1], [5, 5]], np.r_[eye, eye], np.r_[info, info]),
        "a NaN node": lambda: e.poseGraphAddNodes(nan_Z),
        "corrections with an unknown id": lambda: e.poseGraphCorrections([0, 24], np.r_[eye, eye]),
        "corrections before any optimize": lambda: e.poseGraphCorrections([0]),
        "an unknown id in set_fixed": lambda: e.poseGraphSetFixed([2, 99], [1, 1]),
        "a pose that is not finite": lambda: e.poseGraphSetPoses(3, nan_Z),
    }
    for what, call in calls.items():
        with pytest.raises(ng.NgicpError) as err:
            call()
        assert err.value.code == ERR_ARG, what
        assert _same_graph(_snapshot(e), keep), what
    # n == 0 and the caps, through the C ABI (refused before an array is read)
    L, h = e._L, e._h
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int)
    one_T, one_L, one_ij = np.eye(4).reshape(-1), np.eye(6).reshape(-1), np.array([0, 1], np.int32)
    first = C.c_int(-7)
    assert L.ngicp_pose_graph_add_nodes(h, one_T.ctypes.data_as(f64p), None, 0, C.byref(first)) == ERR_ARG
    assert L.ngicp_pose_graph_add_nodes(h, one_T.ctypes.data_as(f64p), None, pgm.MAX_NODES - 24 + 1, C.byref(first)) == ERR_ARG
    assert L.ngicp_pose_graph_add_edges(h, one_ij.ctypes.data_as(i32p), one_T.ctypes.data_as(f64p), one_L.ctypes.data_as(f64p), None, 0, C.byref(first)) == ERR_ARG
    assert L.ngicp_pose_graph_add_edges(h, one_ij.ctypes.data_as(i32p), one_T.ctypes.data_as(f64p), one_L.ctypes.data_as(f64p), None, pgm.MAX_EDGES - 24 + 1,
                                        C.byref(first)) == ERR_ARG
    assert first.value == -7 and _same_graph(_snapshot(e), keep)
    # a component without a fixed node: optimize refuses; the poses stay
    e.poseGraphSetFixed([0], [0])
    with pytest.raises(ng.NgicpError) as err:
        e.poseGraphOptimize()
    assert err.value.code == ERR_ARG and "fixed" in str(err.value)
    assert np.array_equal(e.poseGraphPoses(), keep[1])
    first_new = e.poseGraphAddNodes(np.eye(4))  # a lone free node is a component of its own
    e.poseGraphSetFixed([0], [1])
    with pytest.raises(ng.NgicpError):
        e.poseGraphOptimize()
    e.poseGraphSetFixed([first_new], [1])
    assert e.poseGraphOptimize(**pc.OPTIONS)["accepted"] >= 1  # and with every component gauged it runs
    e.poseGraphClear()
    assert e.poseGraphSize() == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- 7. isolation
def test_an_optimize_leaves_the_alignment_state_bit_for_bit(ng):
    w = clouds.scan_to_scan(4000)
    e = ng.NanoGICP()
    e.setMaxCorrespondenceDistance(1.0)
    e.setInputSource(w.source)
    e.setInputTarget(w.target)
    e.align()
    before = (e.getFinalTransformation().copy(), [a.copy() for a in e.correspondences()], e.getSourceCovariances().copy(), e.getFinalHessian().copy())
    g, _ = pc.ring24()
    e.poseGraphAddNodes(g.poses, g.fixed)
    e.poseGraphAddEdges(g.ij, g.Z, g.info)
    assert e.poseGraphOptimize(**pc.OPTIONS)["accepted"] >= 2
    e.poseGraphCorrections(np.arange(24))
    after = (e.getFinalTransformation(), e.correspondences(), e.getSourceCovariances(), e.getFinalHessian())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3])
    assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
    e.align()
    fresh = ng.NanoGICP()
    fresh.setMaxCorrespondenceDistance(1.0)
    fresh.setInputSource(w.source)
    fresh.setInputTarget(w.target)
    fresh.align()
    fresh.align()
    assert np.array_equal(e.getFinalTransformation(), fresh.getFinalTransformation()) and np.array_equal(e.getFinalHessian(), fresh.getFinalHessian())
    assert np.array_equal(e.getFinalTransformation(), before[0])


# ---------------------------------------------------------------------------------------------------------------- 8. end to end
def test_loop_closure_end_to_end_graph_corrections_keyframes(ng):
    """Twelve small keyframes added at drifted poses; the graph from ground-truth relative poses plus one loop edge; the corrections applied to
    the store.  The corrections equal the model's T_new T_old^-1 rounded to float bit for bit (the model spells the engine's order of
    operations), the moved store equals tests/_keyframe_move_model.py applied to the same matrices, and the optimised poses are the ground
    truth within the optimiser's tolerance."""
    scene = clouds.make_scene()
    truth = pc.truth_walk(12, 31)
    start = pc.drifted(truth, 31)
    prod, store = ng.NanoGICP(), ng.NanoGICP()
    for k in range(12):
        pts = clouds.scan(scene, clouds.make_pose((0.5 * k, 0.2 * k, 1.0), (0.0, 0.0, 7.0 * k)), rings=8, cols=45, elev_deg=(-15.0, 15.0), noise_seed=k)
        prod.setInputSource(pts)
        assert 300 <= len(pts) <= 400 and store.addKeyframeTransformed(prod, start[k].astype(np.float32)) == k
    pairs = pc.chain_pairs(12) + [(11, 0)]
    Z = np.stack([pgm.inv_pose(truth[a]) @ truth[b] for a, b in pairs])
    Z[:, 3] = [0.0, 0.0, 0.0, 1.0]
    info = np.stack([pc.information(np.random.default_rng(50 + e)) for e in range(len(pairs))])
    fixed = np.zeros(12, bool)
    fixed[0] = True
    store.poseGraphAddNodes(start, fixed)
    store.poseGraphAddEdges(pairs, Z, info, np.r_[np.zeros(11, bool), True])
    res = store.poseGraphOptimize(max_iterations=40, rot_eps=1e-9, trans_eps=1e-9, cg_tol=1e-8, cg_max_iterations=2000)
    new = store.poseGraphPoses()
    ids = np.arange(12)
    Cs = store.poseGraphCorrections(ids)
    assert Cs.dtype == np.float32 and np.array_equal(Cs, pgm.corrections(new, start))
    assert np.array_equal(store.poseGraphCorrections([5, 2], start[[5, 2]]), Cs[[5, 2]])  # the caller's T_old, any order of ids
    before = [store.getKeyframe(k) for k in range(12)]
    store.transformKeyframes(ids, Cs)
    want = km.move(before, list(ids), Cs)
    for k in range(12):
        got = store.getKeyframe(k)
        assert np.array_equal(got[0], want[k][0]) and np.array_equal(got[1], want[k][1])
    gap = pc.pose_difference(new, truth)
    print(f"  distance from the ground truth {gap:.3g} after {len(res['trace'])} tries, chi2 {res['initial_chi2']:.6g} -> {res['final_chi2']:.3g}")
    assert res["converged"] and gap <= _pose_tolerance("end_to_end")
