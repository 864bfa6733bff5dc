"""The pose prior on the GPU (ngicp_set_pose_prior; csrc/ngicp_math.h prior_row, csrc/ngicp_solve.h lm_solve_body) against the numpy model
of its definition (tests/_prior_model.py, which proves itself in test_prior_model_cpu.py): the two self-tests, the hooks on every
route, whole alignments pass by pass, neutrality, the batch entries, the robust kernel together with the prior, the corridor, and
what is refused."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _pose_prior_worker as worker
import _prior_model as pm
import _robust_model as rm
import _vgicp_model as vm
from _pass_check import H_TOL
from direct_lidar_odometry_amd import clouds
from oracle.numpy_model import so3_exp
from test_gpu_robust import _POOR_GUESS, _REJECT, _close, _f32, _half_negative, _pick, _poses, _rel
from test_prior_model_cpu import ANGLES, check_corridor, corridor_runs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_pose_prior_worker.py")

ROUTES = {"exact": 0, "direct1": 1, "direct7": 7, "rolling": 1}  # neighbourhood K; 0: exact GICP; rolling: DIRECT1 on a rolling map
RES = 1.0
ERR_ARG, ERR_STATE = -2, -3


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture(scope="module")
def data(ng):
    """clouds.scan_to_submap(3008, 2) with the engine's own covariances (k = 20), the model's voxel map built once, and the prior every
    test uses unless it says otherwise: a pose 5 cm and 1 degree from the guess, a full-rank information matrix.  Nothing here is
    changed by a test."""
    w = clouds.scan_to_submap(3008, 2)
    g = ng.NanoGICP()
    g.setInputSource(w.source); g.setInputTarget(w.target)
    g.calculateSourceCovariances(); g.calculateTargetCovariances()
    cs, ct = g.getSourceCovariances(), g.getTargetCovariances()
    g.close()
    Tp = _f32(clouds.make_pose((0.03, -0.04, 0.01), (0.6, -0.4, 0.8)) @ np.asarray(w.guess, np.float64))
    A = np.random.default_rng(8).normal(size=(6, 6))
    return dict(w=w, cs=cs, ct=ct, maps={}, Tp=Tp, Lam=300.0 * (A @ A.T))


def _engine(ng, data, route, src, cs, prior=None, ct=None, gate=None, kernel=None, **settings):
    """-> (engine, producer or None); the rolling route holds the target in a rolling map (one insert at identity)"""
    w = data["w"]
    ct = data["ct"] if ct is None else ct
    g = ng.NanoGICP()
    if ROUTES[route]:
        g.setVoxelResolution(RES)
        g.setNeighborSearchMethod(ROUTES[route])
    else:
        g.setMaxCorrespondenceDistance(w.max_corr_dist if gate is None else gate)
    for name, v in settings.items():
        getattr(g, name)(v)
    g.setInputSource(src); g.setSourceCovariances(cs)
    if route == "rolling":
        g.setVoxelRolling(True)
        prod = ng.NanoGICP()
        prod.setInputSource(w.target); prod.setSourceCovariances(ct)
        g.insertIntoVoxelMap(prod, np.eye(4, dtype=np.float32))
        prod.close()
    else:
        g.setInputTarget(w.target); g.setTargetCovariances(ct)
    if kernel is not None:
        g.setRobustKernel(*kernel)
    if prior is not None:
        g.setPosePrior(*prior)
    return g


def _model(data, route, src, cs, prior=None, ct=None, tag=None, gate=None, kernel=(rm.NONE, 1.0), **kw):
    w = data["w"]
    ct = data["ct"] if ct is None else ct
    if ROUTES[route] == 0:
        m = pm.make_model(0, src, w.target, cs, ct, max_corr_dist=w.max_corr_dist if gate is None else gate, **kw)
    else:
        if tag not in data["maps"]:
            data["maps"][tag] = vm.VoxelMap(np.asarray(w.target, np.float32), ct, RES)
        m = pm.make_model(ROUTES[route], src, w.target, cs, ct, vmap=data["maps"][tag], **kw)
    m.set_kernel(*kernel)
    return m.set_prior(*prior) if prior is not None else m


def _prior(data):
    return data["Tp"], data["Lam"]


def _corr(g, route):
    """what the model's corr (exact, DIRECT1) or corr_n (DIRECT7) is compared with"""
    return g.voxel_correspondences() if ROUTES[route] > 1 else g.correspondences()[0]


def _model_corr(m, route):
    return m.corr_n if ROUTES[route] > 1 else m.corr


# ---- 1. the self-tests ----------------------------------------------------------------------------------------------------------------------
def _rotvecs():
    """angle x axis: exactly 0, both sides of so3_exp's, so3_log's and the Jacobian's switches, ordinary angles, up to 3 rad"""
    rng = np.random.default_rng(2)
    axes = rng.normal(size=(160, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    angles = np.r_[ANGLES, 1e-3 * (1 + np.array([-1e-3, 1e-3])), 0.1 * (1 + np.array([-1e-6, 1e-6])), rng.uniform(0, 3.0, 8)]
    return np.array([th * ax for th in angles for ax in axes])


def _rowclose(got, ref, what):
    """the small-routine bound of tests/test_gpu_parity.py: rtol 1e-9, atol 1e-12"""
    err = np.abs(got - ref)
    print(f"{what}: {len(ref)} problems, max abs error {err.max():.2e}, max error / (1e-12 + 1e-9 |ref|) {(err / (1e-12 + 1e-9 * np.abs(ref))).max():.2e}")
    assert np.isfinite(got).all() and (err <= 1e-12 + 1e-9 * np.abs(ref)).all(), what


def test_selftest_so3_log_matches_the_model(ng):
    g = ng.NanoGICP()
    W = _rotvecs()
    R = np.array([so3_exp(w) for w in W])
    got = g.mathSelftest(4, R.reshape(-1, 9))
    ref = np.array([pm.so3_log(r) for r in R])
    assert len(W) > 3000 and not got[:160].any()  # (angle exactly 0: phi exactly 0)
    _rowclose(got, ref, "so3_log")
    _rowclose(got, W, "so3_log(so3_exp(w)) vs w")
    # beyond the domain (pi, and R = -I's neighbours): finite
    far = np.array([so3_exp(np.pi * np.array([0, 0, 1.0])), np.diag([-1.0, -1.0, 1.0]), so3_exp(np.array([3.1, 0.2, 0.0]))])
    assert np.isfinite(g.mathSelftest(4, far.reshape(-1, 9))).all()
    g.close()


def test_selftest_prior_row_matches_the_model(ng):
    """poses T = (exp(w) R_p, t) for the same rotation vectors w, random prior poses and full-rank information matrices of size ~ 10"""
    g = ng.NanoGICP()
    W = _rotvecs()
    rng = np.random.default_rng(6)
    probs, ref = [], []
    for w in W:
        Tp = clouds.make_pose(rng.uniform(-3, 3, 3), rng.uniform(-60, 60, 3)).astype(np.float64)
        T = np.eye(4)
        T[:3, :3] = so3_exp(w) @ Tp[:3, :3]
        T[:3, 3] = Tp[:3, 3] + rng.uniform(-0.5, 0.5, 3)
        A = rng.normal(size=(6, 6))
        Lam = A @ A.T
        probs.append(np.r_[T[:3, :3].ravel(), T[:3, 3], Tp[:3, :3].ravel(), Tp[:3, 3], Lam.ravel()])
        ref.append(pm.prior_row(T, Tp, Lam))
    got = g.mathSelftest(5, np.array(probs))
    assert got.shape == (len(W), 28)
    _rowclose(got, np.array(ref), "prior_row")
    g.close()


def test_pose_prior_terms_match_the_model_and_the_getter_returns_the_setting(ng, data):
    g = ng.NanoGICP()
    assert g.getPosePrior() is None
    with pytest.raises(ng.NgicpError) as e:
        g.pose_prior_terms(np.eye(4))
    assert e.value.code == ERR_STATE
    Tp, Lam = _prior(data)
    g.setPosePrior(Tp, Lam)
    T, L = g.getPosePrior()
    assert np.array_equal(T, Tp) and np.array_equal(L, Lam)
    for P in _poses(data["w"]) + (Tp,):
        r, c, H, b = g.pose_prior_terms(P)
        rm_, cm, Hm, bm = pm.prior_terms(P, Tp, Lam)
        _rowclose(np.r_[r, c, H.ravel(), b], np.r_[rm_, cm, Hm.ravel(), bm], "pose_prior_terms")
        assert np.array_equal(H, H.T)
    r, c, H, b = g.pose_prior_terms(Tp)
    assert not r[3:].any() and np.abs(r[:3]).max() <= 1e-15 and c <= 1e-25
    g.clearPosePrior()
    assert g.getPosePrior() is None
    g.close()


# ---- 2. the hooks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src", (1, 255, 256, 257, 3008))
@pytest.mark.parametrize("route", list(ROUTES))
def test_linearize_and_compute_error_match_the_model(ng, data, route, n_src):
    """linearize at the guess and at a pose near the solution, compute_error at a third pose: correspondences exact; H, b and err within
    1e-9 of their largest entry (tests/test_gpu_robust.py's bound).  At T = T_p the difference from the H without a prior is the
    model's J_p^T L J_p, to 1e-9 of H's largest entry (the difference of two sums that large carries that much)."""
    w = data["w"]
    src, cs = _pick(data, n_src)
    prior = _prior(data)
    g = _engine(ng, data, route, src, cs, prior=prior)
    m = _model(data, route, src, cs, prior=prior)
    P0, P1, P2 = _poses(w)
    label = f"{route} n={n_src}"
    for P in (P0, P1):
        H, b, err = g.linearize(P)
        Hm, bm, em = m.linearize(P)
        assert np.array_equal(_corr(g, route), _model_corr(m, route)), label
        _close(H, Hm, 1e-9, label + " H"); _close(b, bm, 1e-9, label + " b"); _close([err], [em], 1e-9, label + " err")
        assert np.array_equal(H, H.T)
    _close([g.compute_error(P2)], [m.compute_error(P2)], 1e-9, label + " compute_error")
    Tp, Lam = prior
    H1, b1, e1 = g.linearize(Tp)
    g.clearPosePrior()
    H0, b0, e0 = g.linearize(Tp)
    _, cp, Hp, bp = pm.prior_terms(Tp, Tp, Lam)
    d = np.abs((H1 - H0) - Hp).max()
    print(f"{label}: (H with - H without) - J_p^T L J_p at T_p: {d:.2e}, of |H| {d / np.abs(H1).max():.2e}")
    assert d <= 1e-9 * np.abs(H1).max() and np.abs(Hp).max() > 0.0
    g.close()


# ---- 3. whole alignments, pass by pass ------------------------------------------------------------------------------------------------------
_GN = dict(setOptimizer=0, setMaximumIterations=15)
# route -> (source points, {case: (settings, guess, seed of the half-negative target covariances or None, gate)}).  The rejection cases use
# the seed (and, on the exact route, the gate) with which the MODEL, run on the CPU with the prior and these settings, rejects trials and
# accepts later ones; their covariances come from the model's side (vm.plane_covariances) for engine and model.
PASS_CASES = {
    "exact": (257, {"lm": (dict(), None, None, None), "gauss_newton": (_GN, None, None, None), "lm_rejection": (_REJECT, _POOR_GUESS, 11, 1.0)}),
    "direct1": (3008, {"lm": (dict(), None, None, None), "gauss_newton": (_GN, None, None, None), "lm_rejection": (_REJECT, _POOR_GUESS, 11, None)}),
    "direct7": (3008, {"lm": (dict(), None, None, None), "gauss_newton": (_GN, None, None, None), "lm_rejection": (_REJECT, _POOR_GUESS, 16, None)}),
}


@pytest.mark.parametrize("case", ["lm", "gauss_newton", "lm_rejection"])
@pytest.mark.parametrize("route", list(PASS_CASES))
def test_every_pass_of_an_alignment_matches_the_model(ng, data, route, case):
    """tests/test_gpu_robust.py's test of the same name with the prior in the kernel's place: align(max_iter = m) for every m up to the
    full run; at the pose of every trace row's linearisation (the float pose the run of m - 1 iterations returned) the correspondences
    are exact and y0 / yi / H (the summed ones) are within H_TOL (1e-5: the engine evaluates at its double pose, the model at
    double(float(pose))).  The lm_rejection cases (half of the target's voxels with negative definite covariances, a poor guess,
    lambda's factor 1e-15, a hundredth of the information matrix) must reject trials; exact / lm must end with a K4-only pass."""
    n_src, cases = PASS_CASES[route]
    settings, guess, negative, gate = cases[case]
    settings = dict(settings)
    w = data["w"]
    src, cs = _pick(data, n_src)
    ct = data["ct"]
    if negative is not None:
        if "plane" not in data:
            data["plane"] = (vm.plane_covariances(w.source, 20), vm.plane_covariances(w.target, 20))
        cs = data["plane"][0][np.linspace(0, 3007, n_src).astype(int)]
        ct = _half_negative(data, data["plane"][1], seed=negative)
    guess = np.asarray(w.guess if guess is None else guess, np.float32)
    prior = _prior(data)
    if case == "lm_rejection":
        # The poor guess lies 1.8 m from T_p.  With the full matrix the prior's gradient there (2 L r, some 1e4 per metre) turns the float
        # rounding of the pose the model is handed (6e-8 m) into more than H_TOL of the cost: a hundredth of the matrix keeps what the
        # bound was made for - and still a tenth of the cost at the guess.
        prior = (prior[0], 0.01 * prior[1])
    max_iter = settings.pop("setMaximumIterations", 64)
    gn = settings.get("setOptimizer", 1) == 0
    g = _engine(ng, data, route, src, cs, prior=prior, ct=ct, gate=gate, **settings)
    m = _model(data, route, src, cs, prior=prior, ct=ct, tag=f"half_negative{negative}" if negative is not None else None, gate=gate)
    g.setMaximumIterations(max_iter)
    g.align(guess)
    full = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), g.nr_iterations_, g.converged_)
    st = g.stats()
    n_full = g.nr_iterations_ + 1
    acc = full[1][:, 7] if len(full[1]) else np.zeros(0)
    print(f"{route} {case}: {n_full} iterations, converged {g.converged_}, {int((acc == 0).sum())} rejected trials, passes {st['passes']}, search passes {st['search_passes']}")
    if case == "lm_rejection":
        assert (acc == 0).any() and (acc == 1).any(), f"accepted {acc.astype(int).tolist()}"
    if (route, case) == ("exact", "lm"):
        assert g.converged_ and st["search_passes"] < st["passes"], "the alignment did not end with a K4-only pass"
    poses, H_at = [guess], {}
    for k in range(1, n_full + 1):
        where = f"{route} {case}: pass {k} of {n_full}"
        g.setMaximumIterations(k)
        g.align(guess)
        T, Hg, tr = g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.lm_trace().copy()
        P = poses[k - 1].astype(np.float64)
        Hm, _, em = m.linearize(P)
        assert np.array_equal(_corr(g, route), _model_corr(m, route)), f"{where}: correspondences differ"
        H_at[k - 1] = Hm
        rows = tr[tr[:, 0] == k - 1] if len(tr) else tr
        dE = 0.0
        for y0 in rows[:, 2] if len(rows) else []:
            dE = max(dE, _rel(y0, em))
            assert _rel(y0, em) <= H_TOL, f"{where}: y0 {y0!r} vs the model's {em!r}"
        if len(rows) and rows[-1, 7] == 1:
            yo = m.compute_error(T.astype(np.float64))
            dE = max(dE, _rel(rows[-1, 3], yo))
            assert _rel(rows[-1, 3], yo) <= H_TOL, f"{where}: yi {rows[-1, 3]!r} of the accepted trial vs the model's {yo!r}"
        if not gn and len(tr) and tr[-1, 7] == 0:  # ended on a rejected trial: the pose stayed, H is that of the last accepted step
            assert np.array_equal(T, poses[k - 1]), f"{where}: a rejected trial moved the pose"
            n_acc = int(tr[:, 7].sum())
            Href = H_at[n_acc - 1] if n_acc else np.eye(6)
        else:
            Href = Hm
        dH = float(np.abs(Hg - Href).max() / np.abs(Href).max())
        print(f"{where}: |dH|/|H| {dH:.1e}, y0/yi rel. {dE:.1e}")
        assert dH <= H_TOL, f"{where}: |dH|/|H| = {dH:.2e}"
        n_rows = int(np.sum(full[1][:, 0] < k)) if len(full[1]) else 0
        assert tr.shape == (n_rows, 8) and np.array_equal(tr, full[1][:n_rows]), f"{where}: the LM trace is not a prefix of the full run's"
        poses.append(T)
    assert np.array_equal(poses[-1], full[0]) and np.array_equal(Hg, full[2]) and (g.nr_iterations_, g.converged_) == full[3:]
    g.close()


# ---- 4. neutrality --------------------------------------------------------------------------------------------------------------------------
def _outcome(g, route, guess, P1, P2):
    g.align(guess)
    out = [g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), np.array([g.nr_iterations_, int(g.converged_)]),
           np.asarray(_corr(g, route))]
    H, b, e = g.linearize(P1)
    out += [H, b, np.array([e, g.compute_error(P2)]), np.asarray(_corr(g, route))]
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_no_prior_a_cleared_prior_and_a_zero_information_matrix_change_nothing(ng, data, route):
    """The transform, the trace, the Hessian, the correspondences (and the hooks) are np.array_equal to the plain align's: with
    L = 0 at an arbitrary T_p every sum gains exactly +0.0 (r and J_p are finite), after set-then-clear the pointer is null again."""
    w = data["w"]
    _, P1, P2 = _poses(w)
    plain = _engine(ng, data, route, w.source, data["cs"])
    want = _outcome(plain, route, w.guess, P1, P2)
    assert len(want[1]) > 0
    plain.close()
    g = _engine(ng, data, route, w.source, data["cs"], prior=_prior(data))
    other = _outcome(g, route, w.guess, P1, P2)
    assert not np.array_equal(other[0], want[0]) and not np.array_equal(other[5], want[5])  # the prior did something
    g.clearPosePrior()
    for i, (x, y) in enumerate(zip(_outcome(g, route, w.guess, P1, P2), want)):
        assert np.array_equal(x, y), f"{route}: set then cleared: item {i} differs"
    far = clouds.make_pose((12.0, -7.0, 3.0), (40, -100, 170)).astype(np.float64)
    g.setPosePrior(far, np.zeros((6, 6)))
    for i, (x, y) in enumerate(zip(_outcome(g, route, w.guess, P1, P2), want)):
        assert np.array_equal(x, y), f"{route}: L = 0: item {i} differs"
    g.close()


# ---- 5. the batch entries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 3, 8))
@pytest.mark.parametrize("route", ["exact", "direct7"])
def test_every_batch_lane_equals_the_single_align_with_the_prior(ng, data, route, B):
    w = data["w"]
    src, cs = _pick(data, 3008)
    g = _engine(ng, data, route, src, cs, prior=_prior(data))
    rng = np.random.default_rng(B)
    guesses = np.stack([(clouds.make_pose(rng.uniform(-0.05, 0.05, 3), rng.uniform(-1, 1, 3)) @ np.asarray(w.guess, np.float64)).astype(np.float32) for _ in range(B)])
    singles = []
    for q in guesses:
        g.align(q)
        singles.append((g.getFinalTransformation().copy(), g.converged_, g.nr_iterations_, g.getFinalHessian().copy(), g.lm_trace().copy()))
    g.align(w.guess)
    last = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), np.asarray(_corr(g, route)).copy())
    T, conv, nit, H = (g.alignBatch if route == "exact" else g.alignBatchVoxel)(guesses)
    for i, s in enumerate(singles):
        assert np.array_equal(T[i], s[0]) and bool(conv[i]) == s[1] and int(nit[i]) == s[2] and np.array_equal(H[i], s[3]), f"{route} B={B}: lane {i}"
        assert np.array_equal(g.lm_trace(lane=i), s[4]), f"{route} B={B}: trace of lane {i}"
    now = (g.getFinalTransformation(), g.lm_trace(), g.getFinalHessian(), _corr(g, route))
    for a, b in zip(now, last):
        assert np.array_equal(a, b), "the batch changed what the last align's getters return"
    # and the prior reached the lanes: without it lane 0 ends elsewhere
    g.clearPosePrior()
    T0 = (g.alignBatch if route == "exact" else g.alignBatchVoxel)(guesses)[0]
    assert not np.array_equal(T0[0], T[0])
    g.close()


# ---- 6. the robust kernel and the prior together --------------------------------------------------------------------------------------------
def test_a_robust_kernel_and_the_prior_together_match_the_model(ng, data):
    """DIRECT1, Cauchy of width 1: the hooks to 1e-9, and the prior's share unchanged by the kernel (it is not re-weighted): the
    difference between linearize with and without the prior is the same H_p under the kernel."""
    w = data["w"]
    src, cs = _pick(data, 3008)
    prior, kernel = _prior(data), (rm.CAUCHY, 1.0)
    g = _engine(ng, data, "direct1", src, cs, prior=prior, kernel=kernel)
    m = _model(data, "direct1", src, cs, prior=prior, kernel=kernel)
    P0, P1, P2 = _poses(w)
    for P in (P0, P1):
        H, b, err = g.linearize(P)
        Hm, bm, em = m.linearize(P)
        assert np.array_equal(_corr(g, "direct1"), _model_corr(m, "direct1"))
        _close(H, Hm, 1e-9, "H"); _close(b, bm, 1e-9, "b"); _close([err], [em], 1e-9, "err")
    _close([g.compute_error(P2)], [m.compute_error(P2)], 1e-9, "compute_error")
    assert (m.last_w[m.last_s > 0] < 0.9).any()  # the kernel is at work
    g.align(w.guess)
    T = g.getFinalTransformation()
    Tm = m.align(w.guess)
    dt, dr = clouds.pose_error(T, Tm)
    print(f"robust + prior align: engine vs model {dt:.2e} m / {dr:.2e} rad, iterations {g.nr_iterations_ + 1} vs {m.nr_iterations + 1}")
    assert dt <= 1e-4 and dr <= 1e-4 and g.nr_iterations_ == m.nr_iterations
    g.close()


# ---- 7. the corridor ------------------------------------------------------------------------------------------------------------------------
def test_the_corridor_on_the_engine(ng):
    """test_prior_model_cpu.py's case on the engine: the final float transform equals the model's (the model is handed the engine's
    inputs: the same clouds and covariances), and both orderings hold for the engine's own numbers."""
    models = {}

    def run_model(c, prior):
        m = pm.make_model(0, c["src"], c["tgt"], c["cs"], c["ct"], max_corr_dist=1.0)
        if prior:
            m.set_prior(*prior)
        models[prior is not None] = (m.align(c["guess"]), m.nr_iterations)
        return models[prior is not None][0]

    def run_engine(c, prior):
        g = ng.NanoGICP()
        g.setMaxCorrespondenceDistance(1.0)
        g.setInputSource(c["src"]); g.setInputTarget(c["tgt"])
        g.setSourceCovariances(c["cs"]); g.setTargetCovariances(c["ct"])
        if prior:
            g.setPosePrior(*prior)
        g.align(c["guess"])
        T, it = g.getFinalTransformation().copy(), g.nr_iterations_
        assert g.converged_
        g.close()
        Tm, itm = models[prior is not None]
        print(f"corridor, prior {prior is not None}: engine vs model max |dT| {np.abs(T - Tm).max():.2e}, iterations {it + 1} vs {itm + 1}")
        assert np.array_equal(T, Tm) and it == itm, "the engine's final transform is not the model's"
        return T

    corridor_runs(run_model)
    plain, prior = corridor_runs(run_engine)
    check_corridor(plain, prior)


# ---- 8. arguments and refusals --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_and_refused_entries_keep_the_former_prior(ng, data):
    w = data["w"]
    src, cs = _pick(data, 257)
    Tp, Lam = _prior(data)
    g = _engine(ng, data, "exact", src, cs, prior=(Tp, Lam))
    g.align(w.guess)
    want = g.getFinalTransformation().copy()

    def bad(T, L):
        with pytest.raises(ng.NgicpError) as e:
            g.setPosePrior(T, L)
        assert e.value.code == ERR_ARG and "pose prior" in str(e.value), str(e.value)
        T1, L1 = g.getPosePrior()
        assert np.array_equal(T1, Tp) and np.array_equal(L1, Lam)

    for v in (np.nan, np.inf, -np.inf):
        T = Tp.copy(); T[1, 3] = v
        bad(T, Lam)
        L = Lam.copy(); L[2, 2] = v
        bad(Tp, L)
        L = Lam.copy(); L[1, 4] = L[4, 1] = v
        bad(Tp, L)
    T = Tp.copy(); T[3, 1] = 1e-30
    bad(T, Lam)
    T = Tp.copy(); T[3, 3] = 1.0 + 2.0 ** -52
    bad(T, Lam)
    L = Lam.copy(); L[0, 5] = np.nextafter(L[0, 5], np.inf)
    bad(Tp, L)
    L = np.diag([1.0, 1.0, -1e-300, 1.0, 1.0, 1.0])
    bad(Tp, L)
    g.align(w.guess)
    assert np.array_equal(g.getFinalTransformation(), want)
    with pytest.raises(ng.NgicpError) as e:
        g.sharded_begin(w.guess)
    assert e.value.code == ERR_ARG and "pose prior" in str(e.value)
    # the hooks' state stays valid across a change of the prior
    g.linearize(Tp)
    g.setPosePrior(Tp, 2.0 * Lam)
    e2 = g.compute_error(Tp)
    g.clearPosePrior()
    assert g.compute_error(Tp) <= e2
    # the setting survives mode switches
    g.setPosePrior(Tp, Lam)
    g.setVoxelResolution(RES); g.setNeighborSearchMethod(7); g.setVoxelResolution(0.0)
    T1, L1 = g.getPosePrior()
    assert np.array_equal(T1, Tp) and np.array_equal(L1, Lam)
    g.align(w.guess)
    assert np.array_equal(g.getFinalTransformation(), want)
    g.clearPosePrior()
    g.sharded_begin(w.guess)  # available again
    g.close()


@pytest.fixture(scope="module")
def default_route(ng, tmp_path_factory):
    """what the default route returns for the worker's inputs, with the prior and without"""
    g, w, Tp, Lam = worker.setup(ng, clouds)
    T0 = worker.outcome(g, w)[0]
    g.setPosePrior(Tp, Lam)
    T, trace, H = worker.outcome(g, w)
    g.close()
    assert not np.array_equal(T, T0) and len(trace) > 0
    path = str(tmp_path_factory.mktemp("pose_prior") / "default_route.npz")
    np.savez(path, T=T, trace=trace, H=H, T0=T0)
    return path


# every switch whose optimiser steps in lm_solve_body applies the prior; k_gicp_head steps in every block from its own sums: refused
SWITCHES = {"NGICP_PASS_IMPL": "applied", "NGICP_FUSED": "applied", "NGICP_QUEUE": "applied", "NGICP_PERSIST": "applied", "NGICP_SERIAL_STEP": "applied",
            "NGICP_HEAD": "refused"}


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_an_align_under_a_kernel_variant_switch_applies_the_prior_or_is_refused(hip_lib, default_route, switch):
    """The switches are read once per process, so each runs in a child of its own (tests/_pose_prior_worker.py): the align with the
    prior equals the default route's bit for bit (RESULT applied) or is refused naming the pose prior (RESULT refused); a switch that
    ignores the prior fails in the worker.  Which of the two each switch does is the table above (include/ngicp.h states it)."""
    env = dict(os.environ, **{switch: "1"})
    res = subprocess.run([sys.executable, WORKER, default_route], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert f"RESULT {SWITCHES[switch]}" in res.stdout, res.stdout[-2000:]
