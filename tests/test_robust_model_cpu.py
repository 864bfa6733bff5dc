"""The numpy model of the robust kernels (tests/_robust_model.py) proving itself without a GPU: w is the derivative of rho, the kernels
reduce to the plain cost where they must, H and b are the derivatives of the robust cost, a vast width reproduces the plain models, and
the kernels do what they are for on a scan of which a sector has moved."""
import numpy as np
import pytest

import _robust_model as rm
import _vgicp_model as vm
import _vgicp_nbr_model as nbm
from direct_lidar_odometry_amd import clouds
from oracle.numpy_model import NumpyGICP
from test_vgicp_model_cpu import _perturbed

KINDS = sorted(rm.KINDS)


def _ids(k):
    return rm.NAMES[k]


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
@pytest.mark.parametrize("c", [0.5, 1.0, 3.0])
def test_w_is_the_derivative_of_rho(kind, c):
    """Central differences with a relative step h = 1e-5 on s.  Truncation: every rho is piecewise analytic with |rho'''| s^2 <= 6 |rho'|
    (Huber's outer branch 2 c sqrt(s): 3/4; Cauchy: 2 s^2 / (c2 + s)^2 <= 2; Geman-McClure: 6 s^2 / (c2 + s)^2 <= 6), so it is below
    h^2 w.  Rounding: the two values of rho carry an error of a few eps rho each (4 eps taken for the pair and the operations inside),
    divided by 2 h s - where rho saturates (Geman-McClure, large s) that term is what is left.  The bound is their sum, fixed from
    this.  Points within 4 h of Huber's knee are left out: the difference quotient straddles the two branches there."""
    s = np.geomspace(1e-6, 1e6, 4001)
    h = 1e-5
    if kind == rm.HUBER:
        s = s[np.abs(s / (c * c) - 1.0) > 4 * h]
    up, _ = rm.rho_w(s * (1 + h), kind, c)
    dn, _ = rm.rho_w(s * (1 - h), kind, c)
    rho, w = rm.rho_w(s, kind, c)
    fd = (up - dn) / (2 * h * s)
    bound = h * h * w + 4 * np.finfo(float).eps * rho / (2 * h * s)
    print(f"{rm.NAMES[kind]} c={c}: |fd - w| at most {(np.abs(fd - w) / bound).max():.2f} of the bound, {(np.abs(fd - w) / w).max():.1e} of w")
    assert (np.abs(fd - w) <= bound).all()
    assert ((w > 0) & (w <= 1)).all() and (np.diff(w) <= 0).all()  # a weight, never growing with s


def test_huber_is_continuous_at_the_knee_and_every_kernel_is_the_plain_cost_for_small_s():
    for c in (0.5, 1.0, 3.0):
        c2 = c * c
        lo, hi = np.nextafter(c2, 0.0), np.nextafter(c2, np.inf)
        (r0, r1, r2), (w0, w1, w2) = rm.rho_w(np.array([lo, c2, hi]), rm.HUBER, c)
        assert r1 == c2 and w1 == 1.0 and w0 == 1.0 and r0 == lo  # s <= c2 is the inlier branch
        assert abs(r2 - c2) <= 4 * np.spacing(c2) and abs(w2 - 1.0) <= 4 * np.spacing(1.0)
        for kind in rm.KINDS:
            s = c2 * np.array([1e-12, 1e-10, 1e-9])
            rho, w = rm.rho_w(s, kind, c)
            # rho = s (1 - O(s / c2)), w = 1 - O(s / c2) with constants 1 and 2 at most (Geman-McClure's); 3 leaves room for rounding
            assert (np.abs(rho - s) <= 3 * (s / c2) * s).all() and (np.abs(w - 1) <= 3 * s / c2).all(), rm.NAMES[kind]


@pytest.mark.parametrize("kind", (rm.NONE,) + rm.KINDS, ids=_ids)
def test_a_term_that_is_not_positive_passes_through(kind):
    s = np.array([0.0, -0.0, -1e-300, -3.5, -1e300, np.nan])
    rho, w = rm.rho_w(s, kind, 0.7)
    assert np.array_equal(rho, s, equal_nan=True) and (w == 1).all()
    assert rm.rho_w(np.array([2.0]), rm.NONE, 0.7)[0][0] == 2.0


def _models(seed=0):
    """One small scene under the three routes: exact (a random symmetric positive definite set, a gate that leaves some points out),
    DIRECT1 and DIRECT7.  The residuals are spread so that every kernel of width 1 sees terms on both sides of s = c2."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-6, 6, (1500, 3)).astype(np.float32)
    A = rng.normal(0, 0.1, (1500, 3, 3))
    ct = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    src = (tgt[rng.permutation(1500)[:300]] + rng.normal(0, 0.05, (300, 3))).astype(np.float32)
    B = rng.normal(0, 0.1, (300, 3, 3))
    cs = B @ B.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    c4s, c4t = np.zeros((300, 4, 4)), np.zeros((1500, 4, 4))
    c4s[:, :3, :3], c4t[:, :3, :3] = cs, ct
    return {
        "exact": (lambda cls=rm.RobustNumpyGICP: cls(src, tgt, c4s, c4t, max_corr_dist=0.12)),
        "direct1": (lambda cls=rm.RobustVoxelGICPModel: cls(src, tgt, cs, ct, 1.0)),
        "direct7": (lambda cls=rm.RobustVoxelGICPNbrModel: cls(src, tgt, cs, ct, 1.0, neighbors=7)),
    }


_T0 = clouds.make_pose((0.05, -0.02, 0.03), (0.5, -0.4, 0.8))


@pytest.mark.parametrize("route", ["exact", "direct1", "direct7"])
@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_b_is_half_the_gradient_of_the_robust_cost(route, kind):
    """At fixed correspondences and matrices, cost(d) = sum rho(s(d)) at the pose delta(d) * T has the gradient sum w 2 J^T M e = 2 b at
    d = 0 (J = d e / d d for the left-multiplied step, as tests/test_vgicp_model_cpu.py states for the plain cost; the sign follows
    from e = b - T a).  Central differences with step h.  Unlike the plain cost, which is quadratic in e, rho(s) bends on the scale of
    the residual itself: a step moves a point by up to h (1 + r) (r: the cloud's radius), and the relative truncation error of a term
    is of the order of (h (1 + r) / |e|)^2, with constants of at most 6 from the kernels' derivatives (test_w_is_the_derivative_of_rho).
    Terms with |e| below 1 cm - a fifth of the scene's 5 cm noise - carry a correspondingly small share of b, so |e| = 1 cm is taken:
    with h = 1e-6 the bound is 6 (h (1 + r) / 0.01)^2, about 1e-5 of the largest entry of b.  Rounding adds 8 eps cost / (2 h).
    Huber's second derivative jumps at the knee: a term that crosses it within the step may be off by its whole share, so the bound
    carries the fraction of such terms, which is counted, not assumed (none is expected at this h)."""
    width = 0.5 if route == "exact" else 1.0  # (the exact route's gate of 12 cm keeps s small: a narrower kernel has terms on both sides)
    c2 = width * width
    g = _models()[route]().set_kernel(kind, width)
    H, b, err = g.linearize(_T0)
    s = g.last_s[g.last_s >= 0]
    assert (s > c2).sum() >= 10 and (s < c2).sum() >= 10, "the case must have terms on both sides of s = c2"
    assert np.abs(H - H.T).max() <= 1e-15 * np.abs(H).max()
    h = 1e-6
    r = float(np.abs(g.src).max() * np.sqrt(3))
    tol = 6 * (h * (1.0 + r) / 0.01) ** 2 + 8 * np.finfo(float).eps * abs(err) / (2 * h) / np.abs(b).max()
    grad = np.empty(6)
    near = 0
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        up = g.compute_error(_perturbed(_T0, d))
        s_up = g.last_s.copy()
        dn = g.compute_error(_perturbed(_T0, -d))
        near = max(near, int((((s_up > c2) != (g.last_s > c2)) & (s_up >= 0)).sum()))
        grad[k] = (up - dn) / (2 * h)
    if kind == rm.HUBER:
        tol += near / len(s)
    print(f"{route} {rm.NAMES[kind]}: b vs FD {np.abs(grad / 2 - b).max() / np.abs(b).max():.2e}, tolerance {tol:.2e}, {near} terms crossed the knee")
    assert np.abs(grad / 2 - b).max() <= tol * np.abs(b).max()
    assert abs(g.compute_error(_T0) - err) <= 1e-12 * abs(err)


@pytest.mark.parametrize("route", ["exact", "direct1", "direct7"])
def test_a_vast_width_and_none_reproduce_the_plain_model(route):
    """Width 1e150 (c2 = 1e300 is finite): Huber never leaves its inlier branch and is the plain cost exactly; Cauchy and Geman-McClure
    have s / c2 < 1e-290, which rounds away.  The plain model is the parent class on the same data; its sums are taken in another order
    (a loop or one einsum per slot), hence 1e-12 of the largest entry rather than bits."""
    plain_cls = {"exact": NumpyGICP, "direct1": vm.VoxelGICPModel, "direct7": nbm.VoxelGICPNbrModel}[route]
    p = _models()[route](plain_cls)
    Hp, bp, ep = p.linearize(_T0)
    T2 = _perturbed(_T0, [1e-3, -2e-3, 5e-4, 0.01, -0.02, 0.005])
    e2p = p.compute_error(T2) if hasattr(p, "compute_error") else p.accumulate(T2, want=False)[2]
    for kind, width in [(rm.NONE, 1.0)] + [(k, 1e150) for k in rm.KINDS]:
        g = _models()[route]().set_kernel(kind, width)
        H, b, e = g.linearize(_T0)
        e2 = g.accumulate(T2, want=False)[2]
        assert np.array_equal(g.corr, p.corr)
        assert np.abs(H - Hp).max() <= 1e-12 * np.abs(Hp).max() and np.abs(b - bp).max() <= 1e-12 * np.abs(bp).max()
        assert abs(e - ep) <= 1e-12 * ep and abs(e2 - e2p) <= 1e-12 * e2p
        assert (g.last_w[g.last_s >= 0] == 1).all() or kind != rm.HUBER


@pytest.fixture(scope="module")
def scenario():
    """clouds.scan_to_submap(3008, 2) at 1 m with the 512 source points of azimuth (0.2, 0.2 + pi / 3) shifted by (0.35, 0.25, 0) m;
    the plain DIRECT1 model's outcome is computed once."""
    w = clouds.scan_to_submap(3008, 2)
    src, sel = rm.outlier_scenario(w)
    cs, ct = vm.plane_covariances(src, 20), vm.plane_covariances(w.target, 20)
    kw = dict(max_iter=32, trans_eps=1e-4, rot_eps=1e-4)
    first = rm.RobustVoxelGICPModel(src, w.target, cs, ct, 1.0, **kw)

    def run(kind, width=1.0):
        m = rm.RobustVoxelGICPModel.__new__(rm.RobustVoxelGICPModel)
        NumpyGICP.__init__(m, src, w.target, cs, ct, **kw)
        m.vmap = first.vmap  # built once
        m.set_kernel(kind, width)
        T = m.align(w.guess)
        return m, T, clouds.pose_error(T, w.gt)[0]

    return dict(w=w, sel=sel, run=run, plain=run(rm.NONE))


def test_the_scenario_moves_512_points_and_the_plain_model_is_pulled_off(scenario):
    assert int(scenario["sel"].sum()) == 512
    m, _, dt = scenario["plain"]
    print(f"none: {dt:.4f} m from ground truth after {m.nr_iterations + 1} iterations, converged {m.converged}")
    assert dt > 0.05 and m.converged


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_every_kernel_of_width_1_ends_within_a_third_of_the_plain_error(scenario, kind):
    """The figures this was written down with: none 0.0737 m; Huber 0.0137, Cauchy 0.0045, Geman-McClure 0.0015 (ratios 0.19, 0.06,
    0.02)."""
    _, _, plain = scenario["plain"]
    m, T, dt = scenario["run"](kind)
    m.update_correspondences(T.astype(np.float64))
    m.accumulate(T.astype(np.float64))
    sel, has = scenario["sel"], m.last_s[:, 0] >= 0
    print(f"{rm.NAMES[kind]}: {dt:.4f} m ({dt / plain:.2f} of none's {plain:.4f}), {m.nr_iterations + 1} iterations, converged {m.converged}; "
          f"mean w {m.last_w[sel & has].mean():.3f} on the shifted points, {m.last_w[~sel & has].mean():.3f} on the rest")
    assert m.converged and dt <= plain / 3
    assert m.last_w[sel & has].mean() < m.last_w[~sel & has].mean()
