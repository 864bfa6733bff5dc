"""The robust kernels on the GPU (ngicp_set_robust_kernel; csrc/ngicp_terms.h robust_term, csrc/ngicp_robust.h) against the numpy model
of their definition (tests/_robust_model.py, which proves itself in test_robust_model_cpu.py): the hooks on every route, whole
alignments pass by pass, the bit anchors to the code without a kernel, ngicp_robust_terms, the outlier scenario, the rolling map, and
what is refused."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _robust_model as rm
import _vgicp_model as vm
from _pass_check import H_TOL
from direct_lidar_odometry_amd import clouds
from oracle.numpy_model import NumpyGICP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_robust_worker.py")

ROUTES = {"exact": 0, "direct1": 1, "direct7": 7, "direct27": 27}  # neighbourhood K; 0: exact GICP
SIZES = (1, 37, 257, 3008)  # around the 256-thread block, the 32-query batch of the exact pass and the probe loops
RES = 1.0
ERR_ARG = -2


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture(scope="module")
def data(ng):
    """clouds.scan_to_submap(3008, 2) with the engine's own covariances (k = 20); the model's voxel maps are built once per set of
    target covariances and shared.  Nothing here is changed by a test."""
    w = clouds.scan_to_submap(3008, 2)
    g = ng.NanoGICP()
    g.setInputSource(w.source); g.setInputTarget(w.target)
    g.calculateSourceCovariances(); g.calculateTargetCovariances()
    cs, ct = g.getSourceCovariances(), g.getTargetCovariances()
    g.close()
    return dict(w=w, cs=cs, ct=ct, maps={})


def _pick(data, n):
    idx = np.linspace(0, 3007, n).astype(int) if n < 3008 else np.arange(3008)
    return np.ascontiguousarray(data["w"].source[idx]), data["cs"][idx]


def _engine(ng, data, route, src, cs, kernel=None, ct=None, gate=None, tgt=None, **settings):
    w = data["w"]
    g = ng.NanoGICP()
    if ROUTES[route]:
        g.setVoxelResolution(RES)
        g.setNeighborSearchMethod(ROUTES[route])
    else:
        g.setMaxCorrespondenceDistance(w.max_corr_dist if gate is None else gate)
    for name, v in settings.items():
        getattr(g, name)(v)
    g.setInputSource(src); g.setInputTarget(w.target if tgt is None else tgt)
    g.setSourceCovariances(cs); g.setTargetCovariances(data["ct"] if ct is None else ct)
    if kernel is not None:
        g.setRobustKernel(*kernel)
    return g


def _model(data, route, src, cs, kernel=(rm.NONE, 1.0), ct=None, tag=None, gate=None, **kw):
    w = data["w"]
    ct = data["ct"] if ct is None else ct
    if ROUTES[route] == 0:
        m = rm.RobustNumpyGICP(src, w.target, cs, ct, max_corr_dist=w.max_corr_dist if gate is None else gate, **kw)
    else:
        m = rm.RobustVoxelGICPNbrModel.__new__(rm.RobustVoxelGICPNbrModel)
        NumpyGICP.__init__(m, src, w.target, cs, ct, **kw)
        if tag not in data["maps"]:
            data["maps"][tag] = vm.VoxelMap(m.tgt, ct, RES)
        m.vmap = data["maps"][tag]
        m.set_neighbors(ROUTES[route])
    return m.set_kernel(*kernel)


def _corr(g, route):
    """what the model's corr (exact, DIRECT1) or corr_n (DIRECT7 / 27) is compared with"""
    return g.voxel_correspondences() if ROUTES[route] > 1 else g.correspondences()[0]


def _model_corr(m, route):
    return m.corr_n if ROUTES[route] > 1 else m.corr


def _f32(T):
    """a pose whose entries are exactly float-representable: the engine (double in) and the model evaluate the same one"""
    return np.asarray(T, np.float64).astype(np.float32).astype(np.float64)


def _close(a, b, tol, what):
    scale = np.abs(b).max()
    d = np.abs(np.asarray(a) - np.asarray(b)).max()
    print(f"{what}: off by {d / scale if scale else d:.2e} of the largest entry")
    assert d <= tol * scale, what


def _half_negative(data, ct, seed=11):
    """The target covariances ct with those of about half of the target's VOXELS replaced by -2 I (tests/test_gpu_vgicp.py's
    construction): M is negative definite there, !(s > 0) passes through the kernel, a step from a poor guess goes uphill and LM
    rejects trials.  On the exact route the same set makes every second correspondence or so a negative one."""
    ijk = vm.voxel_of(data["w"].target, RES)
    key = ijk[:, 0] + 4096 * (ijk[:, 1] + 4096 * ijk[:, 2])
    uk = np.unique(key)
    neg = uk[np.random.default_rng(seed).random(len(uk)) < 0.5]
    ct = ct.copy()
    ct[np.isin(key, neg), :3, :3] = -2.0 * np.eye(3)
    return ct


_SAVED = ("corr", "sqd", "mahal", "q", "corr_n")


def _poses(w):
    """The guess (6 cm from the solution); a pose some 18 cm and 2 degrees from it; a third a small step from the second.  Chosen on the
    CPU model so that 37 points already have terms on both sides of c2 = 0.25 and of c2 = 9 on every route (the exact route's gate of
    0.5 m keeps s small at the guess)."""
    P0 = _f32(w.guess)
    P1 = _f32(clouds.make_pose((0.12, -0.1, 0.08), (1, 0.5, -2)) @ w.gt)
    P2 = _f32(clouds.make_pose((0.01, -0.02, 0.005), (0.1, 0.05, -0.2)) @ P1)
    return P0, P1, P2


# ---- 1. model parity of the hooks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src", SIZES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_linearize_and_compute_error_match_the_model(ng, data, route, n_src):
    """linearize at the guess and at a pose near the solution, then compute_error at a third pose, for every kind and the widths 0.5
    and 3.0: correspondences (voxel numbers) exact; H, b and err within 1e-9 of their largest entry - the project's bar for H and b in
    test_gpu_vgicp.py.  The model's correspondences do not depend on the kernel and are taken once per pose.  In every case of 37
    points or more the model must see terms on both sides of s = c2 (asserted): a case that never leaves the inlier branch proves
    nothing."""
    w = data["w"]
    src, cs = _pick(data, n_src)
    g = _engine(ng, data, route, src, cs)
    m = _model(data, route, src, cs)
    P0, P1, P2 = _poses(w)
    saved = []
    for P in (P0, P1):
        m.update_correspondences(P)
        saved.append({k: getattr(m, k) for k in _SAVED if hasattr(m, k)})
    for kind in rm.KINDS:
        for width in (0.5, 3.0):
            g.setRobustKernel(kind, width)
            m.set_kernel(kind, width)
            label = f"{route} n={n_src} {rm.NAMES[kind]} {width}"
            s_seen = []
            for P, state in zip((P0, P1), saved):
                for k, v in state.items():
                    setattr(m, k, v)
                H, b, err = g.linearize(P)
                Hm, bm, em = m.accumulate(P)
                s_seen.append(m.last_s[m.last_s > 0])
                assert np.array_equal(_corr(g, route), _model_corr(m, route)), label
                _close(H, Hm, 1e-9, label + " H"); _close(b, bm, 1e-9, label + " b"); _close([err], [em], 1e-9, label + " err")
                assert np.array_equal(H, H.T)
            e2, e2m = g.compute_error(P2), m.compute_error(P2)
            s_seen.append(m.last_s[m.last_s > 0])
            _close([e2], [e2m], 1e-9, label + " compute_error")
            s_all = np.concatenate(s_seen)
            print(f"{label}: {(s_all <= width * width).sum()} terms at or below c2, {(s_all > width * width).sum()} above")
            if n_src >= 37:
                assert (s_all <= width * width).any() and (s_all > width * width).any(), label + ": terms on one side of c2 only"
    g.close()


# ---- 2. whole alignments, pass by pass ----------------------------------------------------------------------------------------------------
_POOR_GUESS = clouds.make_pose((1.5, -1.0, 0.2), (2, -3, 12)).astype(np.float32)
_REJECT = dict(setMaximumIterations=12, setInitialLambdaFactor=1e-15)  # _pass_check.CASES["lm_rejection"]'s settings
# route -> (source points, {case: (settings, guess, kernel, half-negative target covariances, gate)}).  The rejection cases use the
# kernel with which the MODEL, run on the CPU with these settings, rejects trials, accepts one, and rejects again later; so that the run
# on the CPU says what the engine will meet, their covariances come from the model's side (vm.plane_covariances) for engine and model.
PASS_CASES = {
    "exact": (257, {
        "lm": (dict(), None, (rm.CAUCHY, 1.0), False, None),
        "gauss_newton": (dict(setOptimizer=0, setMaximumIterations=15), None, (rm.HUBER, 1.0), False, None),
        "lm_rejection": (_REJECT, _POOR_GUESS, (rm.GEMAN_MCCLURE, 3.0), True, 2.0),
    }),
    "direct1": (3008, {
        "lm": (dict(), None, (rm.GEMAN_MCCLURE, 1.0), False, None),
        "gauss_newton": (dict(setOptimizer=0, setMaximumIterations=15), None, (rm.CAUCHY, 1.0), False, None),
        "lm_rejection": (_REJECT, _POOR_GUESS, (rm.CAUCHY, 1.0), True, None),
    }),
    "direct7": (3008, {
        "lm": (dict(), None, (rm.HUBER, 1.0), False, None),
        "gauss_newton": (dict(setOptimizer=0, setMaximumIterations=15), None, (rm.GEMAN_MCCLURE, 1.0), False, None),
        "lm_rejection": (_REJECT, _POOR_GUESS, (rm.HUBER, 1.0), True, None),
    }),
}


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@pytest.mark.parametrize("case", ["lm", "gauss_newton", "lm_rejection"])
@pytest.mark.parametrize("route", list(PASS_CASES))
def test_every_pass_of_an_alignment_matches_the_model(ng, data, route, case):
    """tests/test_gpu_vgicp.py's test of the same name with a robust kernel set: align(max_iter = m) for every m up to the full run; at
    the pose of every trace row's linearisation (the float pose the run of m - 1 iterations returned) the correspondences are exact and
    y0 / yi / H are within H_TOL (1e-5: the engine evaluates at its double pose, the model at double(float(pose))) - the tolerances of
    that test, for the reason it states.  The lm_rejection cases must reject trials (asserted): a rejected trial is followed by an
    error pass that evaluates rho at a new pose on the matrices and correspondences of the linearisation that stayed; yi of the trial
    accepted after rejected ones pins that, against the model's robust error under its frozen linearisation."""
    n_src, cases = PASS_CASES[route]
    settings, guess, kernel, negative, gate = cases[case]
    settings = dict(settings)
    w = data["w"]
    src, cs = _pick(data, n_src)
    ct = data["ct"]
    if negative:
        if "plane" not in data:
            data["plane"] = (vm.plane_covariances(w.source, 20), vm.plane_covariances(w.target, 20))
        cs = data["plane"][0][np.linspace(0, 3007, n_src).astype(int)]
        ct = _half_negative(data, data["plane"][1])
    guess = np.asarray(w.guess if guess is None else guess, np.float32)
    max_iter = settings.pop("setMaximumIterations", 64)
    gn = settings.get("setOptimizer", 1) == 0
    g = _engine(ng, data, route, src, cs, kernel=kernel, ct=ct, gate=gate, **settings)
    m = _model(data, route, src, cs, kernel=kernel, ct=ct, tag="half_negative" if negative else None, gate=gate)
    g.setMaximumIterations(max_iter)
    g.align(guess)
    full = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), g.nr_iterations_, g.converged_)
    n_full = g.nr_iterations_ + 1
    acc = full[1][:, 7] if len(full[1]) else np.zeros(0)
    print(f"{route} {case} {rm.NAMES[kernel[0]]}: {n_full} iterations, converged {g.converged_}, {int((acc == 0).sum())} rejected trials")
    if case == "lm_rejection":
        assert (acc == 0).any() and (acc == 1).any(), f"accepted {acc.astype(int).tolist()}"
        assert (acc[1:][acc[:-1] == 0] == 1).any(), "no trial was accepted right after a rejected one"
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
    f = _engine(ng, data, route, src, cs, kernel=kernel, ct=ct, gate=gate, **settings)  # a fresh handle: bit-identical
    f.setMaximumIterations(max_iter)
    f.align(guess)
    assert np.array_equal(f.getFinalTransformation(), full[0]) and np.array_equal(f.lm_trace(), full[1]) and np.array_equal(f.getFinalHessian(), full[2])
    g.close(); f.close()


# ---- 3. bit anchors -----------------------------------------------------------------------------------------------------------------------
def _outcome(g, route, guess, P1, P2):
    g.align(guess)
    out = [g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), np.array([g.nr_iterations_, int(g.converged_)]),
           *[np.asarray(x) for x in g.correspondences()]]
    H, b, e = g.linearize(P1)
    out += [H, b, np.array([e, g.compute_error(P2)]), np.asarray(_corr(g, route))]
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_huber_of_width_1e150_is_none_bit_for_bit(ng, data, route):
    """c2 = 1e300 is finite and above every s: each term takes Huber's inlier branch, w = 1.0 and rho = s exactly, and the robust
    instantiation - other code objects than the default ones, which run for NONE - must produce the same bits: the final transform,
    the LM trace, the Hessian, the iteration count, linearize, compute_error and the correspondences."""
    w = data["w"]
    _, P1, P2 = _poses(w)
    a = _engine(ng, data, route, w.source, data["cs"])
    b = _engine(ng, data, route, w.source, data["cs"], kernel=(rm.HUBER, 1e150))
    assert b.getRobustKernel() == (ng.RobustKernel.HUBER, 1e150) and a.getRobustKernel()[0] == ng.RobustKernel.NONE
    for i, (x, y) in enumerate(zip(_outcome(a, route, w.guess, P1, P2), _outcome(b, route, w.guess, P1, P2))):
        assert np.array_equal(x, y), f"{route}: item {i} differs"
    assert len(a.lm_trace()) > 0
    a.close(); b.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_setting_a_kind_and_then_none_restores_the_default_results(ng, data, route):
    w = data["w"]
    _, P1, P2 = _poses(w)
    g = _engine(ng, data, route, w.source, data["cs"])
    want = _outcome(g, route, w.guess, P1, P2)
    g.setRobustKernel(ng.RobustKernel.GEMAN_MCCLURE, 1.0)
    other = _outcome(g, route, w.guess, P1, P2)
    assert not np.array_equal(other[0], want[0]) and not np.array_equal(other[6], want[6])  # the kernel did something
    g.setRobustKernel(ng.RobustKernel.NONE)
    assert g.getRobustKernel() == (ng.RobustKernel.NONE, 1.0)  # (NONE has no width: the last one stays)
    for i, (x, y) in enumerate(zip(_outcome(g, route, w.guess, P1, P2), want)):
        assert np.array_equal(x, y), f"{route}: item {i} differs"
    g.close()


# ---- 4. robust_terms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", (rm.NONE,) + rm.KINDS, ids=lambda k: rm.NAMES[k])
@pytest.mark.parametrize("route,n_src", [("exact", 3008), ("exact", 37), ("direct1", 3008), ("direct7", 257), ("direct7", 3008), ("direct27", 3008), ("direct27", 1)])
def test_robust_terms_match_the_model_term_by_term(ng, data, route, n_src, kind):
    """After a linearisation at P1, at the pose P2: shapes (n, 1) / (n, 7) / (n, 27); the marker -1 / 0 exactly where the slot has no
    correspondence; s and w within 1e-12 of the model's value of the same term, relative to it; sum rho(s) over the terms within 1e-12
    of compute_error(P2), relative; with NONE every w is 1 and sum s is compute_error(P2) to the same bound.  The source carries three
    points outside every voxel and beyond the gate."""
    w = data["w"]
    src, cs = _pick(data, n_src)
    far = np.array([[500, 500, 500], [3e5, 0, 0], [0.3, 0.2, 40.0]] if ROUTES[route] else [[60, 60, 60], [-70, 50, 30], [0.3, 0.2, 40.0]], np.float32)
    src = np.ascontiguousarray(np.r_[src, far])
    cs = np.r_[cs, np.repeat(np.diag([0.01, 0.02, 0.03, 0.0])[None], 3, 0)]
    width = 1.0
    g = _engine(ng, data, route, src, cs, kernel=(kind, width))
    m = _model(data, route, src, cs, kernel=(kind, width))
    _, P1, P2 = _poses(w)
    g.linearize(P1)
    m.linearize(P1)
    s, wt = g.robust_terms(P2)
    em = m.compute_error(P2)
    K = max(ROUTES[route], 1)
    assert s.shape == wt.shape == (len(src), K)
    corr = np.asarray(_corr(g, route)).reshape(len(src), K)
    none = corr < 0
    assert np.array_equal(none, m.last_s == -1.0) and none[-3:].all() and (n_src == 1 or (~none).any())
    assert (s[none] == -1.0).all() and (wt[none] == 0.0).all()
    has = ~none
    ds = np.abs(s[has] - m.last_s[has]) / np.abs(m.last_s[has])
    dw = np.abs(wt[has] - m.last_w[has]) / m.last_w[has]
    rho, _ = rm.rho_w(s[has], kind, width)
    e2 = g.compute_error(P2)
    dsum = _rel(float(rho.sum()), e2)
    print(f"{route} n={n_src} {rm.NAMES[kind]}: {has.sum()} terms, s off by {ds.max() if has.any() else 0:.1e}, w by {dw.max() if has.any() else 0:.1e} (relative), "
          f"sum rho vs compute_error {dsum:.1e}, the model's error {_rel(e2, em):.1e}")
    assert (ds <= 1e-12).all() and (dw <= 1e-12).all()
    assert dsum <= 1e-12
    if kind == rm.NONE:
        assert (wt[has] == 1.0).all() and _rel(float(s[has].sum()), e2) <= 1e-12
    else:
        assert n_src < 37 or ((wt[has] < 1.0).any() and (wt[has] > 0.0).all())
    # T = None is the final transformation
    g.align(w.guess)
    s1, w1 = g.robust_terms()
    s2, w2 = g.robust_terms(g.getFinalTransformation().astype(np.float64))
    assert np.array_equal(s1, s2) and np.array_equal(w1, w2)
    g.close()


# ---- 5. it does what it is for ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario(data):
    """The outlier scenario of test_robust_model_cpu.py (512 source points of one sector shifted by (0.35, 0.25, 0) m) with covariances
    from the model's side (vm.plane_covariances), handed to the engine and to the model alike."""
    w = data["w"]
    src, sel = rm.outlier_scenario(w)
    return dict(src=src, sel=sel, cs=vm.plane_covariances(src, 20), ct=vm.plane_covariances(w.target, 20), plain={})


@pytest.mark.parametrize("kind", rm.KINDS, ids=lambda k: rm.NAMES[k])
@pytest.mark.parametrize("route", ["direct1", "exact"])
def test_the_outlier_scenario_on_the_engine(ng, data, scenario, route, kind):
    """Width 1.0, max_iter 32, trans_eps = rot_eps = 1e-4.  The exact route's inputs (the same clouds, the workload's gate of 0.5 m)
    were chosen on the CPU model first: alone it ends 0.0667 m from ground truth without a kernel and 0.0141 / 0.0035 / 0.0008 m with
    Huber / Cauchy / Geman-McClure - at most a third, asserted again here.  The engine's final transform is within 1e-4 m / 1e-4 rad of
    that route's own robust model, and the mean weight of the shifted points is below that of the rest."""
    w = data["w"]
    sc = scenario
    st = dict(setMaximumIterations=32, setTransformationEpsilon=1e-4, setRotationEpsilon=1e-4)
    kw = dict(max_iter=32, trans_eps=1e-4, rot_eps=1e-4)
    if route not in sc["plain"]:
        p = _model(data, route, sc["src"], sc["cs"], ct=sc["ct"], tag="scenario", **kw)
        sc["plain"][route] = clouds.pose_error(p.align(w.guess), w.gt)[0]
    plain = sc["plain"][route]
    m = _model(data, route, sc["src"], sc["cs"], kernel=(kind, 1.0), ct=sc["ct"], tag="scenario", **kw)
    Tm = m.align(w.guess)
    g = _engine(ng, data, route, sc["src"], sc["cs"], kernel=(kind, 1.0), ct=sc["ct"], **st)
    g.align(w.guess)
    T = g.getFinalTransformation()
    dt, dr = clouds.pose_error(T, Tm)
    e_model, e_engine = clouds.pose_error(Tm, w.gt)[0], clouds.pose_error(T, w.gt)[0]
    s, wt = g.robust_terms()
    has, sel = s[:, 0] >= 0, sc["sel"]
    w_in, w_out = wt[has & sel, 0].mean(), wt[has & ~sel, 0].mean()
    print(f"{route} {rm.NAMES[kind]}: engine vs model {dt:.2e} m / {dr:.2e} rad; from ground truth: plain model {plain:.4f} m, robust model {e_model:.4f} m, "
          f"engine {e_engine:.4f} m; iterations {g.nr_iterations_ + 1} vs {m.nr_iterations + 1}; mean w {w_in:.3f} on the shifted points, {w_out:.3f} on the rest")
    assert plain > 0.05 and e_model <= plain / 3
    assert dt <= 1e-4 and dr <= 1e-4
    assert g.converged_ and m.converged
    assert w_in < w_out
    g.close()


# ---- 6. the rolling map ---------------------------------------------------------------------------------------------------------------------
def test_a_robust_align_on_a_rolling_map_equals_the_target_based_one(ng, data):
    """One insert at identity gives the target-based map bit for bit (test_gpu_vgicp_rolling.py); the passes read the same view of
    either, so the robust DIRECT1 alignment, its hooks and robust_terms come out the same bits."""
    w = data["w"]
    _, P1, P2 = _poses(w)
    prod, r = ng.NanoGICP(), ng.NanoGICP()
    r.setVoxelResolution(RES); r.setVoxelRolling(True)
    ref = ng.NanoGICP()
    ref.setVoxelResolution(RES)
    for e in (r, ref):  # (the source is the first cloud either handle indexes: test_gpu_vgicp_rolling.py explains)
        e.setInputSource(w.source); e.setSourceCovariances(data["cs"])
        e.setRobustKernel(ng.RobustKernel.CAUCHY, 2.0)
    prod.setInputSource(w.target); prod.setSourceCovariances(data["ct"])
    r.insertIntoVoxelMap(prod, np.eye(4, dtype=np.float32))
    ref.setInputTarget(w.target); ref.setTargetCovariances(data["ct"])
    out = []
    for e in (r, ref):
        o = _outcome(e, "direct1", w.guess, P1, P2)
        out.append(o + list(e.robust_terms(P2)))
    for i, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(a, b), f"item {i} differs"
    assert r.voxelMapBuilds() == 0 and (out[0][-1] < 1.0).any() and r.getRobustKernel() == (ng.RobustKernel.CAUCHY, 2.0)
    prod.close(); r.close(); ref.close()


# ---- 7. refusals and arguments ------------------------------------------------------------------------------------------------------------
def _raises_arg(ng, fn, *a, needle="robust"):
    with pytest.raises(ng.NgicpError) as e:
        fn(*a)
    assert e.value.code == ERR_ARG and needle in str(e.value), str(e.value)


def test_refused_routes_and_bad_arguments_change_nothing(ng, data):
    w = data["w"]
    src, cs = _pick(data, 257)
    guesses = np.stack([w.guess, w.guess])

    def outcome(g):
        g.align(w.guess)
        return (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), *g.correspondences())

    for route in ("exact", "direct1"):
        g = _engine(ng, data, route, src, cs)
        want = outcome(g)
        # bad arguments: each is NGICP_ERR_ARG and leaves the former setting
        g.setRobustKernel(ng.RobustKernel.CAUCHY, 2.5)
        for kind, width in [(4, 1.0), (-1, 1.0), (1, 0.0), (2, -1.0), (3, float("nan")), (1, float("inf")), (2, -float("inf"))]:
            _raises_arg(ng, g.setRobustKernel, kind, width)
            assert g.getRobustKernel() == (ng.RobustKernel.CAUCHY, 2.5)
        # the refused routes
        if route == "exact":
            _raises_arg(ng, g.alignBatch, guesses)
            _raises_arg(ng, g.sharded_begin, w.guess)
        else:
            _raises_arg(ng, g.alignBatchVoxel, guesses)
        assert g.getRobustKernel() == (ng.RobustKernel.CAUCHY, 2.5)
        g.setRobustKernel(ng.RobustKernel.NONE)
        for a, b in zip(outcome(g), want):
            assert np.array_equal(a, b), route
        # and with NONE they are available again
        (g.alignBatch if route == "exact" else g.alignBatchVoxel)(guesses)
        g.close()


@pytest.mark.parametrize("switch", ["NGICP_PASS_IMPL", "NGICP_FUSED", "NGICP_QUEUE", "NGICP_PERSIST", "NGICP_HEAD"])
def test_an_align_under_a_kernel_variant_switch_is_refused(hip_lib, switch):
    """The switches are read once per process, so each runs in a child of its own (tests/_robust_worker.py, after _variant_worker.py):
    with a kernel set, an exact-route align returns NGICP_ERR_ARG naming the robust kernel, the setting stays, and with NONE the align
    under the same switch equals the one before, bit for bit."""
    env = dict(os.environ, **{switch: "1"})
    res = subprocess.run([sys.executable, WORKER], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "RESULT refused" in res.stdout, res.stdout[-2000:]


# ---- 8. one point, and a source wholly outside the map ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", ["one_point", "outside"])
def test_one_point_and_a_source_outside_the_map(ng, data, route, case):
    """Finite results and correct markers; where there is no correspondence at all nothing differs from NONE, hooks and alignment
    alike (H = b = 0, err = 0)."""
    w = data["w"]
    K = max(ROUTES[route], 1)
    if case == "one_point":
        src, cs = _pick(data, 1)
    else:
        src, cs = _pick(data, 257)
        src = src + np.float32(300)
    g = _engine(ng, data, route, src, cs, kernel=(rm.GEMAN_MCCLURE, 0.5))
    n = _engine(ng, data, route, src, cs)
    _, P1, P2 = _poses(w)
    H, b, e = g.linearize(P1)
    Hn, bn, en = n.linearize(P1)
    s, wt = g.robust_terms(P2)
    e2 = g.compute_error(P2)
    corr = np.asarray(_corr(g, route)).reshape(len(src), K)
    assert s.shape == (len(src), K) and np.isfinite(e2) and np.isfinite(H).all() and np.isfinite(b).all() and np.isfinite(e) and np.isfinite(s).all() and np.isfinite(wt).all()
    assert np.array_equal(s == -1.0, corr < 0) and np.array_equal(wt == 0.0, corr < 0)
    g.align(w.guess); n.align(w.guess)
    assert np.isfinite(g.getFinalTransformation()).all()
    if case == "outside":
        assert (corr < 0).all() and not H.any() and not b.any() and e == 0.0 and e2 == 0.0
        assert np.array_equal(H, Hn) and np.array_equal(b, bn) and e == en
        for x, y in [(g.getFinalTransformation(), n.getFinalTransformation()), (g.lm_trace(), n.lm_trace()), (g.getFinalHessian(), n.getFinalHessian())]:
            assert np.array_equal(x, y, equal_nan=True)
        assert (g.nr_iterations_, g.converged_) == (n.nr_iterations_, n.converged_)
    g.close(); n.close()
