"""Every pass of an alignment against the oracle (-m gpu), not only its two ends.

Passes 2..N run code that the cold linearize() hook never runs: the warm start from the previous correspondence, the rows listed for
batches that went far in the pass before, the measured-cost launch order (rebuilt during the alignment and carried over to the next one
on the same handle), the tpt / mahal ping-pong and K4's error on the previous correspondences.  A wrong neighbour for a few queries of a
late pass moves the final pose by far less than any pose tolerance, so each pass is observed on its own, through the public API only:

  * align(guess) with setMaximumIterations(m) runs exactly the first m outer iterations of the longer alignment (the optimiser never
    looks ahead).  Its float pose P_m = pose_to_colmajor_f(x0) is the pose the next pass searches with (xi_f = (float)x0); P_0 = guess.
  * correspondences() after it are those of the last ADOPTED linearisation, the one at P_{m-1} (the reference's correspondences_ after
    align(): its last linearize(), impl/lsq_registration_impl.hpp:162).
  * getFinalHessian() is the H of the last ACCEPTED step (final_hessian_, :155,203): at P_{m-1} too, except when the alignment ended on
    rejected trials (LM gave up, or a rejected step was already below the epsilons) - x0 then stayed where it was, and the H is that of
    the iteration before.

Pass m is compared with a COLD oracle search at the GPU's own pose, OracleGICP.linearize(P_{m-1}), on the same shared covariances: the
same gate decisions, float32 squared distances bit for bit on every gated-in query (and equal to the distance to the returned index,
recomputed here in float32 in the kernel's order), indices equal except on exact float32 distance ties, and H within 1e-5 relative.  The
LM trace's errors of that iteration are compared too: y0 (the linearisation's own error) with the oracle's linearize(P_{m-1}) error, and
the accepted trial's yi (K4: the trial pose under the previous correspondences and Mahalanobis matrices) with the oracle's
compute_error(P_m) after that linearize, both within 1e-5 relative.  These tolerances cover ONLY the float rounding of the pose: the GPU
evaluates at the double pose, the oracle at double(float(pose)) (observed: |dH|/|H| < 1e-7, y0 / yi < 3e-6).  The exact correspondence
check carries the strictness; the H and error checks are there for a dropped or duplicated batch or a stale Mahalanobis buffer, each of
order 1e-4 or more on the passes where the pose still moves.  (Comparing with the oracle's OWN alignment would not work for late passes: the two drift apart by rounding - the
reason the FIXED20 trace checks elsewhere stop at row 4.)

Besides, the trace of align(max_iter=m) must be the first rows of the full run's, bit for bit, and its pose must equal what a fresh
handle's align(max_iter=m) returns - the launch order a reused handle carries over changes nothing."""
import numpy as np
import pytest

from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

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


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


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

    return dict(H=Ho - Hm + Hp, err=eo - em + ep, ties=len(differ), frac=float(gin.mean()), yi=yi)


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def check_passes(g, o, guess, label, src, tgt, cs, ct, max_iter, gn=False, fresh=None):
    """Runs align(guess) with max_iter, then align(max_iter=m) for every m up to the full run's outer iterations, each pass against the
    oracle (g and o configured alike, with the same covariances).  fresh(): a new handle set up like g, for the launch-order check.
    Leaves g at max_iter.  Returns the per-pass (ties, gated-in fraction, |dH|/|H|, largest relative error of y0 / yi)."""
    guess = np.asarray(guess, np.float32)
    g.setMaximumIterations(max_iter)
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
            for y0 in rows[:, 2]:
                d = _rel(y0, r["err"])
                assert d <= H_TOL, f"{where}: y0 {y0!r} vs the oracle's linearisation error {r['err']!r} ({d:.2e})"
                dE = max(dE, d)
            if rows[-1, 7] == 1:
                yo = r["yi"](T)
                d = _rel(rows[-1, 3], yo)
                assert d <= H_TOL, f"{where}: yi {rows[-1, 3]!r} of the accepted trial vs the oracle's compute_error at P_{m} {yo!r} ({d:.2e})"
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


class Rig:
    """A GPU handle and an oracle on the same clouds, settings and (the GPU's) covariances, and a factory of fresh GPU handles."""

    def __init__(self, ng, orc, src, tgt, k, gate, settings, tgt_sizes=None, covs=None, tuning=None):
        self.ng, self.src, self.tgt, self.k, self.gate, self.settings, self.tuning = ng, src, tgt, k, gate, dict(settings), tuning
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

    def run(self, guess, label, fresh=True):
        return check_passes(self.g, self.o, guess, label, self.src, self.tgt, self.cs, self.ct, self.max_iter, self.gn,
                            self.handle if fresh else None)


def _scan_to_scan_rig(ng, orc, case):
    w = clouds.scan_to_scan(10_000)
    settings, gate = CASES[case]
    settings = dict(settings)
    k = settings.pop("setCorrespondenceRandomness", 20)
    return Rig(ng, orc, w.source, w.target, k, gate, settings), (REJECTION_GUESS if case == "lm_rejection" else w.guess)


# ------------------------------------------------------------------ 10k scan-to-scan
@pytest.mark.parametrize("case", list(CASES))
def test_every_pass_scan_to_scan_10k(ng, oracle_mod, case):
    rig, guess = _scan_to_scan_rig(ng, oracle_mod, case)
    rig.run(guess, case)
    print(f"{case}: {int((rig.g.lm_trace()[:, 7] == 0).sum())} rejected trials")


@pytest.mark.parametrize("switch", [("NGICP_PERSIST", "1"), ("NGICP_HEAD", "1"), ("NGICP_CELL_BOXES", "1"), ("NGICP_CHUNK", "64")], ids=lambda s: s[0])
@pytest.mark.parametrize("case", list(CASES) + ["c3_fixed20"])
def test_every_pass_under_switches(ng, oracle_mod, monkeypatch, case, switch):
    """The same per-pass checks with each per-handle switch (read at ngicp_create).  NGICP_CHUNK=64 keeps 64 (pass, solve) pairs in
    flight: that many stale ones are still on the stream when align() sees `done` and returns."""
    monkeypatch.setenv(*switch)
    if case == "c3_fixed20":
        w = clouds.scan_to_submap(100_000, 5)
        rig, guess = Rig(ng, oracle_mod, w.source, w.target, 20, w.max_corr_dist, FIXED20, w.keyframe_sizes), w.guess
    else:
        rig, guess = _scan_to_scan_rig(ng, oracle_mod, case)
    rig.run(guess, f"{case} {switch[0]}={switch[1]}")


# ------------------------------------------------------------------ adversarial target shapes, small voxel
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


@pytest.mark.parametrize("shape", ["cube", "plane", "lines", "clumps"])
def test_every_pass_adversarial_shapes(ng, oracle_mod, shape):
    """Uniform volume, one dense plane, dense lines, tight clumps, aligned from ~0.3 m / 5 deg off with a 0.1 m voxel: a step crosses
    several cells, so the warm start lies cells away from the new neighbour and listed rows change between passes.  The covariances
    are fixed (isotropic): the search is what is under test, and clouds this degenerate would leave the optimiser to rounding."""
    src, tgt = _shape(shape)
    c = np.diag([0.01, 0.01, 0.01, 0.0])
    covs = (np.repeat(c[None], len(src), 0), np.repeat(c[None], len(tgt), 0))
    rig = Rig(ng, oracle_mod, src, tgt, 20, 1.0, dict(setMaximumIterations=12, setTransformationEpsilon=1e-6, setRotationEpsilon=1e-6),
              covs=covs, tuning=0.1)
    assert rig.g.stats()["voxel_size"] <= 0.1 + 1e-9
    rig.run(clouds.make_pose((0.2, -0.15, 0.15), (2.0, -2.0, 4.0)), shape)


# ------------------------------------------------------------------ full size
def _full(ng, orc, w, k, gate, settings, guess, tgt_sizes, label):
    rig = Rig(ng, orc, w.source, w.target, k, gate, settings, tgt_sizes)
    out = rig.run(guess, label)
    print(f"{label}: ties per pass {[t[0] for t in out]}")
    return out


@pytest.mark.parametrize("gate", [1.0, None])
def test_every_pass_c2_100k(ng, oracle_mod, gate):
    w = clouds.scan_to_scan(100_000)
    _full(ng, oracle_mod, w, 10 if gate else 20, gate, DLO if gate else {}, w.guess, None, f"c2 gate {gate}")


@pytest.mark.parametrize("settings", [DLO, FIXED20], ids=["dlo", "fixed20"])
def test_every_pass_c3_100k_500k(ng, oracle_mod, settings):
    w = clouds.scan_to_submap(100_000, 5)
    _full(ng, oracle_mod, w, 20, w.max_corr_dist, settings, w.guess, w.keyframe_sizes, "c3 " + ("fixed20" if settings is FIXED20 else "dlo"))


@pytest.mark.parametrize("settings", [DLO, FIXED20], ids=["dlo", "fixed20"])
def test_every_pass_c5_250k_2m(ng, oracle_mod, settings):
    w = clouds.scan_to_submap(250_000, 8, shape="os1")
    _full(ng, oracle_mod, w, 20, w.max_corr_dist, settings, w.guess, w.keyframe_sizes, "c5 " + ("fixed20" if settings is FIXED20 else "dlo"))


def test_every_pass_500k_source(ng, oracle_mod):
    from types import SimpleNamespace
    w = clouds.scan_to_submap(100_000, 5)
    inv = np.linalg.inv(np.asarray(w.guess, np.float64)).astype(np.float32)
    _full(ng, oracle_mod, SimpleNamespace(source=w.target, target=w.source), 10, 1.0, DLO, inv, None, "500k source")


@pytest.mark.parametrize("g_rank", [1, 4])
def test_every_pass_c4_ranks(ng, oracle_mod, g_rank):
    w = clouds.scan_to_submap(100_000, 5, seed_offset=1000 * g_rank)
    _full(ng, oracle_mod, w, 20, w.max_corr_dist, FIXED20, w.guess, w.keyframe_sizes, f"c4 rank {g_rank}")


# ------------------------------------------------------------------ sequences on one handle
def test_every_pass_sequences_on_one_handle(ng, oracle_mod):
    """What one alignment leaves on a handle (tpt entries, the launch order, the grid buffers, the listed-rows flags) must not leak into
    the next: two guesses, then a smaller target, a swap of source and target, and the same source set again (covariances kept)."""
    w = clouds.scan_to_scan(10_000)
    rig = Rig(ng, oracle_mod, w.source, w.target, 20, 1.0, DLO)
    g, o = rig.g, rig.o
    rig.run(w.guess, "first guess")
    rig.run(clouds.make_pose((0.3, -0.2, 0.05), (1.0, -1.0, 4.0)), "second guess")
    # a smaller target: any index carried over from the larger one would be out of range or wrong
    small = np.ascontiguousarray(w.target[::3])
    ct_small = rig.ct[::3].copy()
    for e in (g, o):
        e.setInputTarget(small)
        e.setTargetCovariances(ct_small)
    check_passes(g, o, w.guess, "smaller target", w.source, small, rig.cs, ct_small, rig.max_iter)
    # swap source and target (covariances travel with the clouds)
    for e in (g, o):
        e.swapSourceAndTarget()
    inv = np.linalg.inv(np.asarray(g.getFinalTransformation(), np.float64)).astype(np.float32)
    check_passes(g, o, inv, "swapped", small, w.source, ct_small, rig.cs, rig.max_iter)
    for e in (g, o):
        e.swapSourceAndTarget()
    # the same source cloud again: same identity, covariances kept
    g.setInputSource(w.source); o.setInputSource(w.source)
    assert g.sourceCovariancesSize() == len(w.source)
    check_passes(g, o, w.guess, "same source again", w.source, small, rig.cs, ct_small, rig.max_iter)


# ------------------------------------------------------------------ constructed gate and tie cases
def _f32_transform(T, p):
    Tf = np.asarray(T, np.float32)
    p = np.asarray(p, np.float32)
    return np.array([((Tf[r, 0] * p[0] + Tf[r, 1] * p[1]) + Tf[r, 2] * p[2]) + Tf[r, 3] for r in range(3)], np.float32)


def _d2(q, t):
    d = (np.asarray(q, np.float32) - np.asarray(t, np.float32)).astype(np.float32)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _place(q, axis, sign, want):
    """A float32 point at float32 squared distance exactly `want` from q (or None): along `axis` (sign), and where the steps of dx^2 are coarser
    than one ulp of d^2 (they are, a few metres from the origin), with the small remainder made up on a second axis."""
    q = np.asarray(q, np.float32)
    x = np.float32(q[axis] + np.float32(sign * np.sqrt(np.float64(want))))
    for _ in range(64):  # from the closest x inwards, so that the remainder is >= 0
        t = q.copy()
        t[axis] = x
        rest = np.float64(want) - np.float64(_d2(q, t))
        for other in ((axis + 1) % 3, (axis + 2) % 3):
            if rest < 0:
                break
            y0 = np.float32(q[other] + np.float32(np.sqrt(rest)))
            for k in range(-64, 65):
                u = t.copy()
                u[other] = np.float32(y0 + np.float32(k) * np.spacing(y0))
                if _d2(q, u) == want:
                    return u
        x = np.float32(x - np.float32(sign) * np.spacing(x))
    return None  # (rare: a few directions have no such point within reach of the search; the caller takes another)


@pytest.mark.parametrize("gate", [0.5, 0.3])
def test_constructed_gate_and_tie_cases(ng, oracle_mod, gate):
    """Isolated probe queries 12 m above the scan whose only candidates are target points placed so that, at the float pose a given pass
    searches with, the float32 d^2 is one ulp below, equal to (0.5: 0.25 is exact) or nearest to (0.3: 0.09 is not a float), and one ulp
    above the gate^2 (the search prunes at the float bound of gate^2, the gate itself compares in double).  Pass 1 (the guess) also has
    exact duplicates (a tie at every pose, so in every warm pass too) and pairs exactly equidistant from their query.  Passes 2 and 3 get
    boundary probes of their own, built at the GPU's P_1 / P_2 on the side away from where the query was before: still gated out in the
    earlier passes, so that adding them does not move the poses they were built for (checked)."""
    w = clouds.scan_to_scan(10_000)
    rng = np.random.default_rng(7)
    g2 = np.float64(gate) * np.float64(gate)
    near = np.float32(g2)
    below = near if np.float64(near) < g2 else np.nextafter(near, np.float32(0), dtype=np.float32)
    above = near if np.float64(near) > g2 else np.nextafter(near, np.float32(1), dtype=np.float32)
    wants = [below, near, above]
    # group 0: 3 boundary + 3 duplicate + 3 equidistant probes; groups 1 and 2: 3 boundary probes each; all 4 m apart
    probes = [np.array([[dx, dy, 12.0 + 3.0 * grp] for dx in (-4.0, 0.0, 4.0) for dy in (-4.0, 0.0, 4.0)][:9 if grp == 0 else 3], np.float32)
              + rng.uniform(-0.2, 0.2, (9 if grp == 0 else 3, 3)).astype(np.float32) for grp in range(3)]
    src = np.ascontiguousarray(np.concatenate([w.source] + probes))
    n0 = len(w.source)
    c_probe = np.diag([0.01, 0.01, 0.01, 0.0])
    cs = np.concatenate([oracle_mod.covariances(w.source, 20), np.repeat(c_probe[None], len(src) - n0, 0)])
    ct0 = oracle_mod.covariances(w.target, 20)
    settings = dict(setMaximumIterations=6, setTransformationEpsilon=1e-12, setRotationEpsilon=1e-12)
    guess = w.guess
    extra, built = [], []  # probe target points; (group, query row, target row, wanted d2)
    poses = [np.asarray(guess, np.float32)]

    def gpu_poses(tgt, ct, n):
        g = ng.NanoGICP()
        _configure(g, 20, gate, settings)
        g.setInputSource(src); g.setInputTarget(tgt); g.setSourceCovariances(cs); g.setTargetCovariances(ct)
        out = []
        for m in range(1, n + 1):
            g.setMaximumIterations(m)
            g.align(guess)
            out.append(g.getFinalTransformation().copy())
        g.close()
        return out

    for grp in range(3):
        T = poses[grp]
        for j, p in enumerate(probes[grp]):
            q = _f32_transform(T, p)
            before = [_f32_transform(P, p) for P in poses[:grp]]
            if j < 3:  # the gate boundary: of the six axis directions, the one farthest from the query's earlier positions
                best = None
                for axis in range(3):
                    for sign in (1.0, -1.0):
                        t = _place(q, axis, sign, wants[j])
                        if t is None:
                            continue
                        margin = min([_d2(b, t) for b in before], default=np.float32(np.inf))
                        if best is None or margin > best[0]:
                            best = (margin, t)
                assert best is not None and best[0] > g2 * (1 + 1e-5), f"group {grp}: the query has not moved far enough to place its probe ({best[0]!r})"
                built.append((grp, n0 + sum(len(x) for x in probes[:grp]) + j, len(extra), wants[j]))
                extra.append(best[1])
            elif j < 6:  # an exact duplicate pair, well inside the gate
                t = q.copy(); t[j - 3] = np.float32(t[j - 3] + np.float32(0.5 * gate))
                extra += [t, t.copy()]
            else:  # two points exactly equidistant from the query, on both sides of it along one axis
                a = j - 6
                t1, t2 = q.copy(), q.copy()
                t1[a] = np.float32(q[a] + np.float32(0.25 * gate))
                t2[a] = np.float32(q[a] - np.float32(t1[a] - q[a]))
                assert _d2(q, t1) == _d2(q, t2)
                extra += [t1, t2]
        tgt = np.ascontiguousarray(np.concatenate([w.target, np.array(extra, np.float32)]))
        ct = np.concatenate([ct0, np.repeat(c_probe[None], len(extra), 0)])
        poses = [poses[0]] + gpu_poses(tgt, ct, grp + 1)
    # the probes added for a later pass left the earlier poses where they were built
    assert all(np.array_equal(a, b) for a, b in zip(poses[1:], gpu_poses(tgt, ct, 3)))
    rig = Rig(ng, oracle_mod, src, tgt, 20, gate, settings, covs=(cs, ct))
    out = rig.run(guess, f"constructed gate {gate}")
    assert len(out) >= 3
    # each boundary probe sits where it was built in the pass it was built for, and the gate decides on the double gate^2
    o = rig.o
    for grp, row, trow, want in built:
        o.linearize(np.asarray(poses[grp], np.float64))
        co, so = o.correspondences()
        assert so[row] == want, (grp, row, so[row], want)
        assert (co[row] >= 0) == (np.float64(want) < g2), (grp, row, co[row], want)
        assert co[row] in (-1, len(w.target) + trow)
    print(f"gate {gate}: boundary d2 {sorted({float(x) for x in wants})}, ties per pass {[t[0] for t in out]}")
