"""The numpy model of the pose prior (tests/_prior_model.py) proving itself without a GPU: log_SO3 against scipy and as the inverse of
the engine's so3_exp across both Taylor switches, b_p as the derivative of the prior's cost under the engine's left update, H_p
symmetric positive semi-definite, the prior vanishing at its own pose, and what it is for: a corridor, where GICP cannot see along the
axis."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import _prior_model as pm
from direct_lidar_odometry_amd import clouds
from oracle.numpy_model import so3_exp

# angles on both sides of each switch: so3_exp's (theta^2 = 1e-10), so3_log's (sin^2 = 1e-6) and jinv_coeff's (theta^2 = 1e-2)
ANGLES = [0.0, 1e-9, 0.9e-5, 1.1e-5, 0.99e-3, 1.01e-3, 0.0999, 0.1001, 0.5, 1.0, np.pi / 2, 2.0, 2.9, 3.0]


def _axes():
    rng = np.random.default_rng(1)
    a = np.r_[np.eye(3), rng.normal(size=(5, 3))]
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _spd(seed, scale=1.0):
    A = np.random.default_rng(seed).normal(size=(6, 6))
    return scale * (A @ A.T)


@pytest.mark.parametrize("theta", ANGLES)
def test_log_so3_matches_scipy_and_inverts_so3_exp(theta):
    """so3_exp builds R from a quaternion it does not normalise: R is a rotation to a few eps.  scipy orthonormalises before it takes the
    logarithm, so the two agree to a few eps relative to the angle, amplified near pi by 1 / sin(theta) (7 at 3 rad): 1e-13 + 1e-12 of
    the angle covers it; log(exp(w)) = w to the same bound."""
    for ax in _axes():
        w = theta * ax
        R = so3_exp(w)
        phi = pm.so3_log(R)
        ref = Rotation.from_matrix(R).as_rotvec()
        bound = 1e-13 + 1e-12 * theta
        assert np.abs(phi - ref).max() <= bound, (theta, phi, ref)
        assert np.abs(phi - w).max() <= bound, (theta, phi, w)
    if theta == 0.0:
        assert not pm.so3_log(np.eye(3)).any()


def test_log_so3_is_continuous_across_its_switch():
    """just below and just above sin^2(theta) = 1e-6 the two branches agree to 1e-15 (the series' first omitted term is 0.03 s^8 = 3e-26)"""
    ax = _axes()[4]
    for th in (1e-3 * (1 - 1e-6), 1e-3 * (1 + 1e-6)):
        R = Rotation.from_rotvec(th * ax).as_matrix()
        assert np.abs(pm.so3_log(R) - th * ax).max() <= 1e-15


def test_the_inverse_left_jacobian_is_continuous_and_inverts_the_left_jacobian():
    """J_l(phi) = I + (1 - cos t) / t^2 [phi]x + (t - sin t) / t^3 [phi]x^2 in closed form (t >= 0.05 here: no cancellation worth
    speaking of); J_l^{-1} J_l = I to 1e-12.  The coefficient's two branches agree to 1e-13 at the switch: the closed form subtracts
    x cot x, which is 1 - t^2 / 12 and carries the roundings of cos, sin, the division and the product (4 eps = 9e-16 at most), from 1
    and divides by t^2 = 1e-2: 9e-14.  (In J_l^{-1} the coefficient multiplies [phi]x^2 of size t^2: 1e-15 there.)"""
    from oracle.numpy_model import skew
    for th in (0.05, 0.0999, 0.1001, 1.0, 2.0, 3.0):
        for ax in _axes():
            phi = th * ax
            K = skew(phi)
            Jl = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * (K @ K)
            assert np.abs(pm.left_jacobian_inv(phi) @ Jl - np.eye(3)).max() <= 1e-12, th
    lo, hi = pm.jinv_coeff(1e-2 * (1 - 1e-9)), pm.jinv_coeff(1e-2 * (1 + 1e-9))
    assert abs(lo - hi) <= 1e-13 and abs(pm.jinv_coeff(0.0) - 1.0 / 12.0) == 0.0


@pytest.mark.parametrize("theta", [0.0, 0.5e-3, 0.05, 0.3, 1.5, 2.8])
def test_twice_b_is_the_gradient_of_the_cost_under_the_left_update(theta):
    """Central differences of c(d) = r^T L r at (so3_exp(d[0:3]), d[3:6]) * T with step h = 1e-5: truncation h^2 |c'''| / 6, rounding
    eps |c| / h.  With |L| ~ 10, |r| <= 4 and t ~ 5 m, c and its derivatives are below 1e4: the bound 1e-4 of max(1, |2 b|) is two
    orders above both."""
    rng = np.random.default_rng(3)
    Lam = _spd(5)
    for ax in _axes()[:4]:
        Tp = clouds.make_pose(rng.uniform(-5, 5, 3), rng.uniform(-40, 40, 3)).astype(np.float64)
        T = np.eye(4)
        T[:3, :3] = so3_exp(theta * ax) @ Tp[:3, :3]
        T[:3, 3] = Tp[:3, 3] + rng.uniform(-0.5, 0.5, 3)
        r, c, H, b = pm.prior_terms(T, Tp, Lam)
        h = 1e-5
        fd = np.zeros(6)
        for i in range(6):
            d = np.zeros(6)
            d[i] = h
            fd[i] = (pm.prior_terms(pm.left_update(d, T), Tp, Lam)[1] - pm.prior_terms(pm.left_update(-d, T), Tp, Lam)[1]) / (2 * h)
        assert np.abs(fd - 2 * b).max() <= 1e-4 * max(1.0, np.abs(2 * b).max()), (theta, fd, 2 * b)
        assert abs(c - r @ Lam @ r) <= 1e-12 * max(1.0, c)


def test_h_is_symmetric_positive_semidefinite_and_the_prior_vanishes_at_its_pose():
    rng = np.random.default_rng(9)
    for seed in range(6):
        Lam = _spd(seed) if seed % 2 else np.diag([3.0, 3.0, 0.0, 0.0, 0.0, 7.0])  # (full rank, and the planar-motion recipe)
        Tp = clouds.make_pose(rng.uniform(-5, 5, 3), rng.uniform(-60, 60, 3)).astype(np.float64)
        T = clouds.make_pose(rng.uniform(-1, 1, 3), rng.uniform(-30, 30, 3)).astype(np.float64) @ Tp
        r, c, H, b = pm.prior_terms(T, Tp, Lam)
        assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
        assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-12 * np.abs(H).max() and c >= 0.0
        r0, c0, H0, b0 = pm.prior_terms(Tp, Tp, Lam)
        assert not r0[3:].any() and np.abs(r0[:3]).max() <= 1e-15 and c0 <= 1e-28 and np.abs(b0).max() <= 1e-13 * np.abs(H0).max()
    r0, c0, H0, b0 = pm.prior_terms(np.eye(4), np.eye(4), _spd(1))
    assert not r0.any() and c0 == 0.0 and not b0.any()  # exactly zero where R R_p^T is exactly I


def test_prior_row_is_the_triangle_b_and_the_cost():
    Lam, Tp = _spd(2), clouds.make_pose((1, 2, 3), (10, 20, 30)).astype(np.float64)
    T = clouds.make_pose((0.1, 0.2, -0.1), (3, -2, 5)).astype(np.float64) @ Tp
    r, c, H, b = pm.prior_terms(T, Tp, Lam)
    row = pm.prior_row(T, Tp, Lam)
    assert row.shape == (28,) and row[0] == H[0, 0] and row[5] == H[0, 5] and row[6] == H[1, 1] and row[20] == H[5, 5]
    assert np.array_equal(row[21:27], b) and row[27] == c


def test_the_model_without_a_prior_is_its_parent():
    """set_prior(None) and a zero information matrix leave accumulate's values as the robust model's (the kernel NONE: the plain one)"""
    import _robust_model as rm
    c = pm.corridor_case(n=120)
    T = c["guess"].astype(np.float64)
    p = rm.RobustNumpyGICP(c["src"], c["tgt"], c["cs"], c["ct"], max_corr_dist=1.0)
    want = p.linearize(T)
    for prior in (None, (c["gt"], np.zeros((6, 6)))):
        m = pm.make_model(0, c["src"], c["tgt"], c["cs"], c["ct"], max_corr_dist=1.0)
        if prior:
            m.set_prior(*prior)
        for a, b in zip(m.linearize(T), want):
            assert np.array_equal(a, b)


# the corridor case, recorded: 900 scan points, 1 cm noise, the guess 0.3 m off along the axis, the exact route with
# a gate of 1 m, default settings; the axis-only prior at the true pose has the information 1e4 m^-2 (sigma = 1 cm) on x alone
CORRIDOR_WEIGHT = 1e4
CORRIDOR_PLAIN_ALONG = 0.14600   # m: the model's along-axis error without a prior
CORRIDOR_PRIOR_ALONG = 0.00082   # m: with the prior
CORRIDOR_ACROSS = (-0.00438, 0.00022)  # m: the across-axis errors (y, z) of the plain run; the prior run's differ by 0.22 mm at most
TRANS_EPS = 5e-4                 # the convergence test's translation threshold: a run does not resolve the pose more finely


def corridor_runs(make_aligned):
    """-> (errors of the plain run, errors of the prior run), each T[:3, 3] - gt[:3, 3]; make_aligned(case, prior or None) -> T"""
    c = pm.corridor_case()
    out = []
    for prior in (None, pm.axis_prior(c["gt"], CORRIDOR_WEIGHT)):
        T = np.asarray(make_aligned(c, prior), np.float64)
        out.append(T[:3, 3] - c["gt"][:3, 3])
    return out


def check_corridor(plain, prior):
    print(f"corridor: plain run off by {plain} m, prior run by {prior} m; across-axis difference {np.abs(plain[1:] - prior[1:]).max():.2e} m")
    assert abs(prior[0]) < abs(plain[0]), "the prior run does not end closer along the axis"
    assert np.abs(plain[1:] - prior[1:]).max() <= TRANS_EPS, "the across-axis errors of the two runs differ by more than the runs resolve"


def test_the_corridor_on_the_model():
    """Both orderings on the model alone, and the recorded figures (to the digits given)."""
    def run(c, prior):
        m = pm.make_model(0, c["src"], c["tgt"], c["cs"], c["ct"], max_corr_dist=1.0)
        if prior:
            m.set_prior(*prior)
        T = m.align(c["guess"])
        assert m.converged
        return T

    plain, prior = corridor_runs(run)
    check_corridor(plain, prior)
    assert abs(plain[0] - CORRIDOR_PLAIN_ALONG) <= 5e-5 and abs(prior[0] - CORRIDOR_PRIOR_ALONG) <= 5e-5
    assert np.abs(plain[1:] - CORRIDOR_ACROSS).max() <= 5e-5
