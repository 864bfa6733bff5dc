"""The pose graph's numpy model (tests/_pose_graph_model.py; include/ngicp.h "pose graph") proves itself: its analytic
Jacobians against central differences, its Levenberg-Marquardt against ground truth, its conjugate gradients against its direct solve
(the measurement that sets the tolerance of tests/test_gpu_pose_graph.py), and edge_from_alignment against its third-order rule."""
import functools

import numpy as np
import pytest

import _pose_graph_cases as pc
import _pose_graph_model as pgm


def _unit(rng, n=3):
    v = rng.normal(size=n)
    return v / np.linalg.norm(v)


@pytest.mark.parametrize("angle", [1e-9, 1e-6, 0.9e-3, 1.1e-3, 0.02, 0.099, 0.101, 0.7, 1.6, 2.5])
def test_analytic_jacobians_match_central_differences(angle):
    """Residual rotations from 1e-9 to 2.5 rad (1e-3 rad is so3_log's switch kSo3LogTaylorS2, 0.1 rad the left Jacobian's
    kSo3JinvTaylorTh2: both sides of each), translations up to 1 km.  Step 1e-6: the difference formula's own error is about 1e-12 from
    truncation plus 1e-10 from rounding, scaled by the entry's magnitude; asserted at 1e-6 of the block's largest entry."""
    rng = np.random.default_rng(int(angle * 1e9) % 9973)
    h = 1e-6
    worst = 0.0
    for _ in range(12):
        Ti = pgm.make_pose(rng.uniform(-np.pi, np.pi) * _unit(rng), rng.uniform(-1000, 1000, 3))
        Z = pgm.make_pose(rng.uniform(-np.pi, np.pi) * _unit(rng), rng.uniform(-30, 30, 3))
        E = pgm.make_pose(angle * _unit(rng), rng.uniform(-2, 2, 3))
        Tj = Ti @ Z @ E
        r, Ji, Jj = pgm.jacobians(Ti, Tj, Z)
        assert abs(np.linalg.norm(r[:3]) - angle) <= 1e-9 * max(angle, 1e-3)
        Ni, Nj = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Ni[:, k] = (pgm.residual(pgm.left_update(d, Ti), Tj, Z) - pgm.residual(pgm.left_update(-d, Ti), Tj, Z)) / (2 * h)
            Nj[:, k] = (pgm.residual(Ti, pgm.left_update(d, Tj), Z) - pgm.residual(Ti, pgm.left_update(-d, Tj), Z)) / (2 * h)
        for J, N in ((Ji, Ni), (Jj, Nj)):
            for blk in (np.s_[:3, :3], np.s_[3:, :3], np.s_[3:, 3:], np.s_[:3, 3:]):
                scale = max(np.abs(J[blk]).max(), 1.0)
                worst = max(worst, np.abs(J[blk] - N[blk]).max() / scale)
        assert np.array_equal(Ji, -Jj)  # a common left perturbation of both ends leaves T_i^-1 T_j alone: what the kernels rely on
    assert worst <= 1e-6, worst


@functools.lru_cache(maxsize=None)
def _both(name):
    """-> (result and poses of the direct solve, result and poses of the model's own conjugate gradients), computed once"""
    g, truth = pc.CASES[name]()
    g2 = g.copy()
    a = pgm.optimize(g, "direct", **pc.options(name))
    b = pgm.optimize(g2, "pcg", **pc.options(name))
    return a, g.poses, b, g2.poses, truth


def test_lm_with_the_dense_solve_recovers_the_ground_truth_of_a_noise_free_ring():
    g, truth = pc.ring24(noisy=False)
    start = g.poses.copy()
    res = pgm.optimize(g, "direct", **pc.OPTIONS)
    assert pc.pose_difference(start, truth) > 0.3
    assert res["converged"] and res["accepted"] >= 3 and res["final_chi2"] <= 1e-12 * res["initial_chi2"]
    assert pc.pose_difference(g.poses, truth) <= 1e-7, pc.pose_difference(g.poses, truth)
    assert np.array_equal(g.poses[0], start[0])  # the fixed node


@pytest.mark.parametrize("name", list(pc.CASES))
def test_cg_against_the_direct_solve_sets_the_gpu_tolerance(name):
    """The largest pose difference between the model with the direct solve and the model with its own preconditioned conjugate gradients
    at the default cg_tol (1e-8), per fixture of tests/test_gpu_pose_graph.py.  Measured: pair 4.4e-16, three_mid_fixed 4.4e-16,
    chain65 2.8e-14, chain257 2.4e-13, ring24 1.1e-14, star130 4.3e-14, multi_edge 4.4e-16, two_components 1.1e-14, false_edge_cauchy 3.5e-13,
    false_edge_none 2.4e-12 - the largest of these, recorded as pc.MEASURED_CG_DIFF['default'] = 3e-12, times ten is the GPU test's tolerance
    on every fixture but big4097; big4097, stopped after two outer iterations and run at cg_tol = 1e-11 (pc.CASE_OPTIONS says why), 5.6e-9 (recorded 7e-9), times ten is
    its own.  There the two solvers' final chi2 must also agree far inside the 1e-9 the GPU test asks of the engine."""
    a, pa, b, pb, _ = _both(name)
    diff = pc.pose_difference(pa, pb)
    print(f"{name}: direct vs cg pose difference {diff:.3g}; tries {len(a['trace'])}; cg iterations {b['cg_iterations']}")
    key = name if name in pc.MEASURED_CG_DIFF else "default"
    assert diff <= pc.MEASURED_CG_DIFF[key]
    assert [t[4] for t in a["trace"]] == [t[4] for t in b["trace"]] and a["iterations"] == b["iterations"]
    pc.assert_margins(a, pc.options(name))
    if a["final_chi2"] > 1e-12 * a["initial_chi2"]:
        assert abs(a["final_chi2"] - b["final_chi2"]) <= 1e-10 * a["final_chi2"]  # the reference leaves a tenth of the 1e-9 to the engine


def test_the_recorded_tolerance_is_the_measured_one_not_a_wider_one():
    worst = max(pc.pose_difference(_both(n)[1], _both(n)[3]) for n in pc.CASES if n not in pc.MEASURED_CG_DIFF)
    assert worst <= pc.MEASURED_CG_DIFF["default"] <= 4 * worst
    big = pc.pose_difference(_both("big4097")[1], _both("big4097")[3])
    assert big <= pc.MEASURED_CG_DIFF["big4097"] <= 4 * big


def test_a_false_loop_edge_with_and_without_a_robust_kernel():
    """Recorded, not asserted against a number chosen in advance: the distance from the ground truth under NONE (4.7) and under CAUCHY
    (0.14); with no false edge ring24 ends 0.14 from it (the measurements' own noise)."""
    for name in ("false_edge_none", "false_edge_cauchy", "ring24"):
        a, pa, _, _, truth = _both(name)
        print(f"{name}: distance from ground truth {pc.pose_difference(pa, truth):.3g}, chi2 {a['final_chi2']:.6g}, tries {len(a['trace'])}")
        assert a["accepted"] >= 1 and a["final_chi2"] < a["initial_chi2"]
    assert 0 in [t[4] for t in _both("false_edge_none")[0]["trace"]]  # this fixture is the one whose trace holds rejected tries


def test_edge_from_alignment_is_exact_to_second_order():
    """For T_j = exp(d) * T_aligned, r^T Lambda r differs from d^T H d in third order: halving d shrinks the discrepancy by about eight
    (asserted between 6 and 10).  The seed is one for which no drawn direction has a third-order coefficient so small that the fourth
    order shows in the ratio (twenty seeds scanned: most give 7.4 to 8.7 on every draw, a few have one draw at 5.2 or 12.8)."""
    rng = np.random.default_rng(23)
    for _ in range(20):
        A = rng.normal(size=(6, 6))
        H = A @ A.T + 0.5 * np.eye(6)
        Ti = pgm.make_pose(rng.uniform(-np.pi, np.pi) * _unit(rng), 100.0 * _unit(rng) * rng.uniform(0, 1))
        Ta = Ti @ pgm.make_pose(rng.uniform(-1, 1, 3), rng.uniform(-5, 5, 3))
        Z, Lam = pgm.edge_from_alignment(Ti, Ta, H)
        assert np.array_equal(Lam, Lam.T)
        assert np.abs(pgm.residual(Ti, Ta, Z)).max() <= 1e-12
        u = _unit(rng, 6)
        gap = []
        for scale in (1e-3, 5e-4):
            d = scale * u
            r = pgm.residual(Ti, pgm.left_update(d, Ta), Z)
            gap.append(abs(r @ Lam @ r - d @ H @ d))
        assert gap[0] <= 0.2 * (1e-3 * u) @ H @ (1e-3 * u)  # a correction, not the bulk (the lever arm of 100 m enters it)
        assert 6.0 <= gap[0] / gap[1] <= 10.0, gap


def test_the_model_refuses_what_the_header_refuses():
    g, _ = pc.ring24()
    keep = g.copy()
    eye, info = np.eye(4)[None], np.eye(6)[None]
    bad_T = np.eye(4)[None].copy()
    bad_T[0, 3, 0] = 1e-3
    nan_Z = eye.copy()
    nan_Z[0, 1, 2] = np.nan
    asym = info.copy()
    asym[0, 2, 4] = 1e-300
    calls = [lambda: g.add_edges([[3, 3]], eye, info), lambda: g.add_edges([[0, 24]], eye, info), lambda: g.add_edges([[-1, 2]], eye, info),
             lambda: g.add_edges([[0, 1]], nan_Z, info), lambda: g.add_edges([[0, 1]], bad_T, info), lambda: g.add_edges([[0, 1]], eye, asym),
             lambda: g.add_edges(np.zeros((0, 2)), eye[:0], info[:0]), lambda: g.add_nodes(eye[:0]), lambda: g.add_nodes(bad_T),
             lambda: g.add_edges([[0, 1], [5, 5]], np.r_[eye, eye], np.r_[info, info])]
    for c in calls:
        with pytest.raises(pgm.Refused):
            c()
        assert g.n == keep.n and g.m == keep.m
    g.fixed[:] = False
    with pytest.raises(pgm.Refused):
        pgm.optimize(g, "direct")
    assert np.array_equal(g.poses, keep.poses)
