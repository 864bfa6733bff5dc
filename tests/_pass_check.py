"""The per-pass oracle check of tests/test_gpu_passes.py (its docstring explains the method), shared with the tests that run it under
other settings: test_gpu_search_matrix.py (per-handle switches, grid geometry) and _variant_worker.py (process-wide kernel variants).
Not collected by pytest (no test_ prefix)."""
import os
from contextlib import contextmanager

import numpy as np

from direct_lidar_odometry_amd import clouds

DLO = dict(setMaximumIterations=32, setTransformationEpsilon=0.01)
FIXED20 = dict(setMaximumIterations=20, setTransformationEpsilon=1e-12, setRotationEpsilon=1e-12)
H_TOL = 1e-5  # H, and the errors y0 / yi of the LM trace: the GPU evaluates at the double pose, the oracle at double(float(pose))

# the scan-to-scan cases of test_gpu_parity.py (settings, gate)
CASES = {
    "dlo_s2s": (dict(setMaximumIterations=32, setTransformationEpsilon=0.01, setCorrespondenceRandomness=10), 1.0),
    "dlo_s2m": (dict(setMaximumIterations=32, setTransformationEpsilon=0.01, setCorrespondenceRandomness=20), 0.5),
    "defaults": (dict(), None),
    "fixed20": (dict(FIXED20), 1.0),
    "gauss_newton": (dict(setOptimizer=0, setMaximumIterations=15), 1.0),
    "one_iteration": (dict(setMaximumIterations=1), 1.0),
    "lm_rejection": (dict(setMaximumIterations=12, setInitialLambdaFactor=1e-15), 2.0),
}
REJECTION_GUESS = clouds.make_pose((1.5, -1.0, 0.2), (2, -3, 12)).astype(np.float32)


# ------------------------------------------------------------------ the harness
def f32_sqd(T, src, tgt, rows, cols):
    """float32 squared distance between source point rows[i] under the float pose T and target point cols[i], in the kernels' order
    (Eigen's float 4x4 * 4-vector: ((c0*x + c1*y) + c2*z) + c3; then ((dx*dx + dy*dy) + dz*dz), nothing fused)."""
    Tf = np.asarray(T, np.float32)
    p, t = src[rows].astype(np.float32), tgt[cols].astype(np.float32)
    d = [(((Tf[r, 0] * p[:, 0] + Tf[r, 1] * p[:, 1]) + Tf[r, 2] * p[:, 2]) + Tf[r, 3]) - t[:, r] for r in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def point_terms(src, tgt, cs, ct, rows, corr, T, T_eval=None):
    """Sum over `rows` of the per-point terms of H and of the error (impl/nano_gicp_impl.hpp:205-209,232-257,273-296) in float64: the
    Mahalanobis matrices of the linearisation at T, the residuals at T_eval (default T; compute_error evaluates a trial pose under the
    matrices of the last linearisation)."""
    if len(rows) == 0:
        return np.zeros((6, 6)), 0.0
    T = np.asarray(T, np.float64)
    T_eval = T if T_eval is None else np.asarray(T_eval, np.float64)
    R = T[:3, :3]
    M = np.linalg.inv(ct[corr][:, :3, :3] + R @ cs[rows][:, :3, :3] @ R.T)
    ta = src[rows].astype(np.float64) @ T_eval[:3, :3].T + T_eval[:3, 3]
    e = tgt[corr].astype(np.float64) - ta
    J = np.zeros((len(rows), 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0] = -ta[:, 2], ta[:, 1], ta[:, 2]
    J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = -ta[:, 0], -ta[:, 1], ta[:, 0]
    J[:, :, 3:] = -np.eye(3)
    return np.einsum("nri,nrs,nsj->ij", J, M, J), float(np.einsum("ni,nij,nj->", e, M, e))


def pose_rounding_bound(o, src, tgt, corr, T):
    """A bound of |y(X) - y(T)| over every double pose X that rounds to the float pose T (each entry within half an ulp of T's), where
    y(X) = sum e^T M e, e = b - (R a + t), is the error under the oracle's correspondences `corr` and Mahalanobis matrices (o: linearised).
    y is quadratic in X, so y(X) - y(T) = g . dX + sum dX_i^T M_i dX_i exactly (g: the gradient at T, dX_i: the move of point i): the bound
    is |g| . ulp/2 plus sum lambda_max(M_i) |dX_i|^2.  Near the origin it is ~1e-7 of y; 3.6 km out a float ulp of the rotation (6e-8)
    moves a point by 1e-4 m, and the bound reaches 1e-4 of y and more once the alignment has converged onto small residuals."""
    T = np.asarray(T, np.float64)
    rows = np.flatnonzero(corr >= 0)
    M = o.mahalanobis()[rows, :3, :3]
    a = src[rows, :3].astype(np.float64)
    e = tgt[corr[rows], :3].astype(np.float64) - (a @ T[:3, :3].T + T[:3, 3])
    Me = np.einsum("nij,nj->ni", M, e)
    Tf = np.abs(np.asarray(T, np.float32))
    dR, dt = np.spacing(Tf[:3, :3]).astype(np.float64) / 2, np.spacing(Tf[:3, 3]).astype(np.float64) / 2
    first = 2.0 * float((np.abs(Me.T @ a) * dR).sum() + (np.abs(Me.sum(0)) * dt).sum())
    move = np.abs(a) @ dR.T + dt
    return first + float((np.linalg.eigvalsh(M)[:, -1] * (move ** 2).sum(1)).sum())


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def check_pass(where, P, cg, sg, o, src, tgt, cs, ct):
    """One pass of the GPU (its correspondences cg / distances sg, searched at the float pose P) against a cold oracle search at P.
    Returns the oracle's H and error re-based onto the GPU's tie choices ("H", "err"), the number of ties and the gated-in fraction, and a
    function yi(T) giving the oracle's compute_error(T) under these correspondences, re-based the same way.  (o is left linearised at P.)"""
    Ho, _, eo = o.linearize(np.asarray(P, np.float64))
    co, so = o.correspondences()
    gin = co >= 0
    bad = (cg >= 0) != gin
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{where}: gate decision differs at query {i} (GPU {cg[i]} d2 {sg[i]!r}, oracle {co[i]} d2 {so[i]!r}); {int(bad.sum())} queries")
    bad = gin & (sg != so)
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{where}: float32 squared distance differs at query {i} (GPU {cg[i]} d2 {sg[i]!r}, oracle {co[i]} d2 {so[i]!r}); {int(bad.sum())} queries")
    rows = np.flatnonzero(gin)
    own = f32_sqd(P, src, tgt, rows, cg[rows])
    bad = own != sg[rows]
    if bad.any():
        i = int(rows[_first(bad)])
        raise AssertionError(f"{where}: query {i}: the GPU's distance {sg[i]!r} is not that of its own neighbour {cg[i]} ({own[_first(bad)]!r})")
    differ = np.flatnonzero(cg != co)
    if len(differ):  # an index may differ only where two target points are EXACTLY equidistant in float32 (the kd-tree keeps the one it visits first)
        d_o = f32_sqd(P, src, tgt, differ, co[differ])
        bad = d_o != sg[differ]
        if bad.any():
            i = int(differ[_first(bad)])
            raise AssertionError(f"{where}: query {i}: GPU neighbour {cg[i]} (d2 {sg[i]!r}) vs oracle {co[i]} (d2 {d_o[_first(bad)]!r}): not a tie")
    (Hm, em), (Hp, ep) = point_terms(src, tgt, cs, ct, differ, co[differ], P), point_terms(src, tgt, cs, ct, differ, cg[differ], P)

    def yi(T):
        e = o.compute_error(np.asarray(T, np.float64))
        return e - point_terms(src, tgt, cs, ct, differ, co[differ], P, T)[1] + point_terms(src, tgt, cs, ct, differ, cg[differ], P, T)[1]

    return dict(H=Ho - Hm + Hp, err=eo - em + ep, ties=len(differ), frac=float(gin.mean()), yi=yi,
                rounding=lambda T: pose_rounding_bound(o, src, tgt, co, T))


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def check_passes(g, o, guess, label, src, tgt, cs, ct, max_iter, gn=False, fresh=None, prime=None, pose_rounding=False):
    """Runs align(guess) with max_iter, then align(max_iter=m) for every m up to the full run's outer iterations, each pass against the
    oracle (g and o configured alike, with the same covariances).  fresh(): a new handle set up like g, for the launch-order check.
    prime(g, n): called before every align of g (which runs n iterations), to put the handle into a given state; it must leave g's
    settings as it found them, n iterations included.
    pose_rounding: y0 / yi may differ from the oracle's by H_TOL plus pose_rounding_bound (clouds far from the origin, where the float
    rounding of the pose the oracle evaluates at outweighs H_TOL); the correspondences and H are checked as always.
    Leaves g at max_iter.  Returns the per-pass (ties, gated-in fraction, |dH|/|H|, largest relative error of y0 / yi)."""
    guess = np.asarray(guess, np.float32)
    g.setMaximumIterations(max_iter)
    if prime is not None:
        prime(g, max_iter)
    g.align(guess)
    full_T, full_tr, full_H = g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy()
    full_it, full_conv = g.nr_iterations_, g.converged_
    n_full = full_it + 1
    poses = [guess]
    H_at = {}  # oracle H at P_k, re-based onto the GPU's tie choices of that pass
    out = []
    for m in range(1, n_full + 1):
        where = f"{label}: pass {m} of {n_full}"
        g.setMaximumIterations(m)
        if prime is not None:
            prime(g, m)
        g.align(guess)
        T, Hg, tr = g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.lm_trace().copy()
        cg, sg = g.correspondences()
        # (a) the correspondences of the pass at P_{m-1}, against a cold oracle search there
        r = check_pass(where, poses[m - 1], cg, sg, o, src, tgt, cs, ct)
        Ho, ties, frac = r["H"], r["ties"], r["frac"]
        H_at[m - 1] = Ho
        # the errors of the LM trace: y0 of iteration m-1 is the error of this very linearisation (K2/K3); the accepted trial's yi is K4's
        # error at P_m under the correspondences and Mahalanobis matrices of this pass (the rejected trials' poses are not observable)
        rows = tr[tr[:, 0] == m - 1] if len(tr) else tr
        dE = 0.0
        if len(rows):
            tol = H_TOL + (r["rounding"](poses[m - 1]) / abs(r["err"]) if pose_rounding else 0.0)
            for y0 in rows[:, 2]:
                d = _rel(y0, r["err"])
                assert d <= tol, f"{where}: y0 {y0!r} vs the oracle's linearisation error {r['err']!r} ({d:.2e}, tolerance {tol:.2e})"
                dE = max(dE, d)
            if rows[-1, 7] == 1:
                yo = r["yi"](T)
                d = _rel(rows[-1, 3], yo)
                tol = H_TOL + (r["rounding"](T) / abs(yo) if pose_rounding else 0.0)
                assert d <= tol, f"{where}: yi {rows[-1, 3]!r} of the accepted trial vs the oracle's compute_error at P_{m} {yo!r} ({d:.2e}, tolerance {tol:.2e})"
                dE = max(dE, d)
        ended_on_rejection = not gn and len(tr) > 0 and tr[-1, 7] == 0
        if ended_on_rejection:  # x0 stayed: the pose is P_{m-1}; the H is that of the last accepted step
            assert np.array_equal(T, poses[m - 1]), f"{where}: a rejected trial moved the pose"
            n_acc = int(tr[:, 7].sum())
            Href = H_at[n_acc - 1] if n_acc else np.eye(6)
        else:
            Href = Ho
        dH = float(np.abs(Hg - Href).max() / np.abs(Href).max())
        assert dH <= H_TOL, f"{where}: |dH|/|H| = {dH:.2e}"
        # (b) a prefix of the full run (after the oracle checks, so that a failure there names the pass against the oracle first)
        k = int(np.sum(full_tr[:, 0] < m)) if len(full_tr) else 0
        assert tr.shape == (k, 8) and np.array_equal(tr, full_tr[:k]), f"{where}: the LM trace is not the first {k} rows of the full run's"
        if m == n_full:
            assert np.array_equal(T, full_T) and np.array_equal(Hg, full_H) and (g.nr_iterations_, g.converged_) == (full_it, full_conv), f"{where}: differs from the full run"
        if fresh is not None:
            f = fresh()
            f.setMaximumIterations(m)
            f.align(guess)
            assert np.array_equal(f.getFinalTransformation(), T) and np.array_equal(f.lm_trace(), tr), f"{where}: a fresh handle ends elsewhere"
            f.close()
        poses.append(T)
        out.append((ties, frac, dH, dE))
        print(f"{where}: ties {ties}, gated in {frac:.4f}, |dH|/|H| {dH:.1e}, y0/yi rel. {dE:.1e}")
    g.setMaximumIterations(max_iter)
    return out


# ------------------------------------------------------------------ set-up
def _configure(e, k, gate, settings):
    e.setCorrespondenceRandomness(k)
    if gate is not None:
        e.setMaxCorrespondenceDistance(gate)
    for name, v in settings.items():
        getattr(e, name)(v)


@contextmanager
def handle_env(env):
    """The per-handle switches in `env` (read at ngicp_create) set around the block, the process environment restored after it."""
    old = {name: os.environ.get(name) for name in env or {}}
    try:
        os.environ.update(env or {})
        yield
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


class Rig:
    """A GPU handle and an oracle on the same clouds, settings and (the GPU's) covariances, and a factory of fresh GPU handles.
    env: per-handle switches applied around the creation of every GPU handle (None: the process environment as it is)."""

    def __init__(self, ng, orc, src, tgt, k, gate, settings, tgt_sizes=None, covs=None, tuning=None, env=None):
        self.ng, self.src, self.tgt, self.k, self.gate, self.settings, self.tuning = ng, src, tgt, k, gate, dict(settings), tuning
        self.env = dict(env or {})
        self.max_iter = self.settings.pop("setMaximumIterations", 64)
        self.gn = self.settings.get("setOptimizer", 1) == 0
        self.g = self.handle(covs=False)
        if covs is not None:
            self.cs, self.ct = covs
        else:
            self.g.calculateSourceCovariances()
            self.cs = self.g.getSourceCovariances()
            if tgt_sizes is None:
                self.g.calculateTargetCovariances()
                self.ct = self.g.getTargetCovariances()
            else:  # per-keyframe covariances, concatenated, supplied as DLO does
                self.ct = ng.keyframe_covariances(tgt, tgt_sizes, k)
        self.g.setSourceCovariances(self.cs)
        self.g.setTargetCovariances(self.ct)
        self.o = orc.OracleGICP()
        self.o.setNumThreads(16)
        _configure(self.o, k, gate, self.settings)
        self.o.setInputSource(src)
        self.o.setInputTarget(tgt)
        self.o.setSourceCovariances(self.cs)
        self.o.setTargetCovariances(self.ct)

    def handle(self, covs=True):
        with handle_env(self.env):
            g = self.ng.NanoGICP()
        if self.tuning is not None:
            g.setTuning(self.tuning)
        _configure(g, self.k, self.gate, self.settings)
        g.setInputSource(self.src)
        g.setInputTarget(self.tgt)
        if covs:
            g.setSourceCovariances(self.cs)
            g.setTargetCovariances(self.ct)
        return g

    def run(self, guess, label, fresh=True, prime=None, pose_rounding=False):
        return check_passes(self.g, self.o, guess, label, self.src, self.tgt, self.cs, self.ct, self.max_iter, self.gn,
                            self.handle if fresh else None, prime, pose_rounding)

    def first_align_stats(self, guess):
        """stats() of a fresh handle's first alignment (no history: its first pass lists the region rows of every batch)."""
        f = self.handle()
        f.setMaximumIterations(self.max_iter)
        f.align(np.asarray(guess, np.float32))
        s = f.stats()
        f.close()
        return s


def _scan_to_scan_rig(ng, orc, case, tuning=None, env=None):
    w = clouds.scan_to_scan(10_000)
    settings, gate = CASES[case]
    settings = dict(settings)
    k = settings.pop("setCorrespondenceRandomness", 20)
    return Rig(ng, orc, w.source, w.target, k, gate, settings, tuning=tuning, env=env), (REJECTION_GUESS if case == "lm_rejection" else w.guess)


# ------------------------------------------------------------------ adversarial target shapes
def _shape(name):
    rng = np.random.default_rng({"cube": 1, "plane": 2, "lines": 3, "clumps": 4}[name])
    n = 6000
    if name == "cube":
        tgt = rng.uniform(-3, 3, (n, 3))
    elif name == "plane":
        tgt = np.c_[rng.uniform(-4, 4, (n, 2)), 0.002 * rng.standard_normal(n)]
    elif name == "lines":
        t = rng.uniform(-4, 4, n); k = rng.integers(0, 3, n); off = rng.integers(-3, 4, (n, 2)) * 0.5
        tgt = np.zeros((n, 3))
        for ax in range(3):
            m = k == ax
            tgt[m, ax] = t[m]
            tgt[np.ix_(m, [a for a in range(3) if a != ax])] = off[m]
        tgt += 0.001 * rng.standard_normal((n, 3))
    else:
        centres = rng.uniform(-3, 3, (12, 3))
        tgt = centres[rng.integers(0, 12, n)] + 0.01 * rng.standard_normal((n, 3))
    tgt = tgt.astype(np.float32)
    src = (tgt[rng.permutation(n)[:3000]] + rng.normal(0, 0.02, (3000, 3))).astype(np.float32)
    src = np.r_[src, rng.uniform(-5, 5, (300, 3)).astype(np.float32)]
    return src, tgt


SHAPES = ("cube", "plane", "lines", "clumps")
SHAPE_SETTINGS = dict(setMaximumIterations=12, setTransformationEpsilon=1e-6, setRotationEpsilon=1e-6)
SHAPE_GUESS = clouds.make_pose((0.2, -0.15, 0.15), (2.0, -2.0, 4.0))


def _shape_rig(ng, orc, shape, tuning=0.1, env=None):
    """test_every_pass_adversarial_shapes' set-up: fixed isotropic covariances, gate 1 m, a 0.1 m voxel unless told otherwise."""
    src, tgt = _shape(shape)
    c = np.diag([0.01, 0.01, 0.01, 0.0])
    covs = (np.repeat(c[None], len(src), 0), np.repeat(c[None], len(tgt), 0))
    return Rig(ng, orc, src, tgt, 20, 1.0, SHAPE_SETTINGS, covs=covs, tuning=tuning, env=env), SHAPE_GUESS


def _crowded_rig(ng, orc, case, tuning=None, env=None, gate=1.0):
    """crowded_cell / crowded_row (tests/_index_history_cases.py): more than 65 535 target points in one cell / in front of a batch
    box inside a grid row, the voxel pinned, fixed isotropic covariances as in _shape_rig."""
    import _index_history_cases as ic
    voxel, _, guess = ic.CROWDED[case]
    src, tgt = ic.CROWDED_CLOUDS[case]()
    covs = (np.repeat(ic.ISO_COV[None], len(src), 0), np.repeat(ic.ISO_COV[None], len(tgt), 0))
    return Rig(ng, orc, src, tgt, 20, gate, ic.CROWDED_SETTINGS, covs=covs, tuning=voxel if tuning is None else tuning, env=env), guess


def make_rig(ng, orc, case, tuning=None, env=None):
    """(Rig, guess) of a named workload: a 10k scan-to-scan case of CASES, an adversarial shape (0.1 m voxel unless `tuning`),
    c3_fixed20 / c3_dlo (the bench's scan-to-submap, 100k -> 500k, per-keyframe target covariances), or crowded_cell / crowded_row."""
    if case in ("crowded_cell", "crowded_row"):
        return _crowded_rig(ng, orc, case, tuning, env, gate=None)  # no gate: the batches list their region's rows
    if case in SHAPES:
        return _shape_rig(ng, orc, case, 0.1 if tuning is None else tuning, env)
    if case in ("c3_fixed20", "c3_dlo"):
        w = clouds.scan_to_submap(100_000, 5)
        settings = FIXED20 if case == "c3_fixed20" else DLO
        return Rig(ng, orc, w.source, w.target, 20, w.max_corr_dist, settings, w.keyframe_sizes, tuning=tuning, env=env), w.guess
    return _scan_to_scan_rig(ng, orc, case, tuning, env)
