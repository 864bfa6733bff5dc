"""Voxelized GICP on the GPU (ngicp_set_voxel_resolution; csrc/ngicp_voxel.h) against the numpy model of its definition
(tests/_vgicp_model.py, which proves itself in test_vgicp_model_cpu.py): the voxel map, the linearize / compute_error hooks, whole
alignments pass by pass, and what the mode must leave alone."""
import numpy as np
import pytest

import _vgicp_model as vm
from _pass_check import H_TOL
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _spd(n, seed):
    """n random symmetric positive definite 3x3 matrices as (n, 4, 4) covariances."""
    A = np.random.default_rng(seed).normal(0, 0.1, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return out


def _f32_pose(t, rpy):
    """A pose whose entries are exactly float-representable: the engine (double in) and the model evaluate the same one."""
    return clouds.make_pose(t, rpy).astype(np.float32).astype(np.float64)


def _map_engine(ng, tgt, ct, res):
    g = ng.NanoGICP()
    g.setVoxelResolution(res)
    g.setInputTarget(tgt)
    g.setTargetCovariances(ct)
    return g


def _check_map(got, m, label):
    """ijk and counts exact; every mean and covariance entry within 1e-12 of the model's, relative to that entry itself: both sides add
    the same at most few hundred terms in the same order (ascending original index) in IEEE double without fused operations and divide
    once, so they are expected to agree to the bit (printed); the bound is the issue's."""
    ijk, mean, cov, cnt = got
    assert len(ijk) == len(m), f"{label}: {len(ijk)} voxels, the model has {len(m)}"
    assert np.array_equal(ijk, m.ijk) and np.array_equal(cnt, m.count), label
    dm, dc = np.abs(mean - m.mean), np.abs(cov - m.cov)
    print(f"{label}: {len(m)} voxels, largest count {m.count.max()}, mean off by {(dm / np.maximum(np.abs(m.mean), 1e-300)).max():.1e}, "
          f"cov by {(dc / np.maximum(np.abs(m.cov), 1e-300)).max():.1e} (relative), bit-equal: {np.array_equal(mean, m.mean) and np.array_equal(cov, m.cov)}")
    assert (dm <= 1e-12 * np.abs(m.mean)).all() and (dc <= 1e-12 * np.abs(m.cov)).all(), label


def _cube(n, half, seed):
    return np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(np.float32)


def _lattice_planes(res):
    """Points exactly on lattice planes, negative ones included, some twice; and points just below a plane."""
    k = np.arange(-6, 7, dtype=np.float32) * np.float32(res)
    p = np.stack(np.meshgrid(k, k[::3], k[::4], indexing="ij"), -1).reshape(-1, 3)
    below = np.nextafter(p[::5], np.float32(-np.inf))
    return np.ascontiguousarray(np.r_[p, p[::7], below, np.array([[-0.0, 0.0, -0.0]], np.float32)])


def _one_per_voxel():
    c = np.arange(-6, 6, dtype=np.float32) + np.float32(0.5)
    return np.ascontiguousarray(np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)[::-1])  # 1728 voxels, given in descending order


MAP_CASES = {
    **{f"n{n}": (lambda n=n: _cube(n, 3.0, n), 1.0) for n in (1, 63, 64, 65, 1023, 1024, 1025)},
    "n4100_tiles": (lambda: _cube(4100, 10.0, 7), 1.0),          # crosses a radix tile (1024) and a scan tile (4096); > 1024 voxels
    "n8000_res025": (lambda: _cube(8000, 3.0, 8), 0.25),
    "n8000_res4": (lambda: _cube(8000, 30.0, 9), 4.0),
    "one_voxel": (lambda: np.random.default_rng(10).uniform(0.05, 0.95, (700, 3)).astype(np.float32), 1.0),
    "one_voxel_negative": (lambda: np.random.default_rng(11).uniform(-3.9, -0.1, (300, 3)).astype(np.float32), 4.0),
    "one_point_per_voxel": (_one_per_voxel, 1.0),
    "lattice_planes_res1": (lambda: _lattice_planes(1.0), 1.0),
    "lattice_planes_res025": (lambda: _lattice_planes(0.25), 0.25),
    "duplicates": (lambda: np.ascontiguousarray(np.repeat(_cube(300, 2.0, 12), 5, axis=0)[np.random.default_rng(12).permutation(1500)]), 1.0),
}


@pytest.mark.parametrize("case", sorted(MAP_CASES))
def test_voxel_map_matches_the_model(ng, case):
    make, res = MAP_CASES[case]
    tgt = make()
    ct = _spd(len(tgt), 100 + len(tgt))
    m = vm.VoxelMap(tgt, ct, res)
    if case.startswith("one_voxel"):
        assert len(m) == 1
    if case == "one_point_per_voxel":
        assert (m.count == 1).all() and len(m) == 1728
    if case == "n4100_tiles":
        assert len(m) > 1024
    g = _map_engine(ng, tgt, ct, res)
    assert g.getVoxelMapSize() == len(m)
    _check_map(g.voxelMap(), m, case)
    g.close()


def test_voxel_map_follows_resolution_target_and_covariances(ng):
    """The map is rebuilt when any of the three changes, and only what changed differs."""
    tgt = _cube(3000, 5.0, 20)
    ct = _spd(3000, 21)
    g = _map_engine(ng, tgt, ct, 1.0)
    _check_map(g.voxelMap(), vm.VoxelMap(tgt, ct, 1.0), "res 1")
    g.setVoxelResolution(4.0)
    _check_map(g.voxelMap(), vm.VoxelMap(tgt, ct, 4.0), "res 4")
    ct2 = _spd(3000, 22)
    g.setTargetCovariances(ct2)
    _check_map(g.voxelMap(), vm.VoxelMap(tgt, ct2, 4.0), "new covariances")
    tgt2 = _cube(2000, 5.0, 23)
    g.setInputTarget(tgt2)  # clears the covariances: the engine computes them (k = 20)
    got = g.voxelMap()
    c_new = g.getTargetCovariances()
    _check_map(got, vm.VoxelMap(tgt2, c_new, 4.0), "new target")
    g.close()


def test_a_target_beyond_2_pow_20_voxels_is_refused(ng):
    tgt = np.r_[_cube(100, 3.0, 30), np.array([[262144.0, 0, 0]], np.float32)]  # 2^18 m / 0.25 m = 2^20
    g = _map_engine(ng, tgt, _spd(len(tgt), 31), 0.25)
    with pytest.raises(ng.NgicpError) as e:
        g.voxelMap()
    assert e.value.code == -2
    g.setInputSource(_cube(50, 3.0, 32))
    with pytest.raises(ng.NgicpError) as e:
        g.align()
    assert e.value.code == -2
    g.setVoxelResolution(1.0)  # the same cloud at 1 m: |i| = 2^18
    assert g.getVoxelMapSize() == len(vm.VoxelMap(tgt, _spd(len(tgt), 31), 1.0))
    tgt[-1, 0] = -262144.25    # floor(-262144.25 * 4) = -2^20 - 1
    g.setInputTarget(tgt); g.setTargetCovariances(_spd(len(tgt), 31)); g.setVoxelResolution(0.25)
    with pytest.raises(ng.NgicpError):
        g.getVoxelMapSize()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ng.NgicpError) as e:
            g.setVoxelResolution(bad)
        assert e.value.code == -2
    g.close()


def test_the_map_after_swap_is_the_old_source_s(ng):
    src, tgt = _cube(1500, 4.0, 40), _cube(2500, 4.0, 41)
    cs, ct = _spd(1500, 42), _spd(2500, 43)
    g = _map_engine(ng, tgt, ct, 1.0)
    g.setInputSource(src); g.setSourceCovariances(cs)
    _check_map(g.voxelMap(), vm.VoxelMap(tgt, ct, 1.0), "before the swap")
    g.swapSourceAndTarget()
    _check_map(g.voxelMap(), vm.VoxelMap(src, cs, 1.0), "after the swap")
    g.close()


def test_the_map_of_a_device_submap_equals_that_of_the_same_data_from_the_host(ng):
    sc = clouds.make_scene()
    scans = [clouds.vlp16(sc, clouds.make_pose((0.5 * i, 0.2 * i, 0.0), (0, 0, 3.0 * i)), noise_seed=50 + i, cols=150) for i in range(3)]
    prod, g = ng.NanoGICP(), ng.NanoGICP()
    g.setVoxelResolution(1.0)
    for i, s in enumerate(scans):
        prod.setInputSource(s)
        g.addKeyframeTransformed(prod, clouds.make_pose((0.5 * i, 0.2 * i, 0.0), (0, 0, 3.0 * i)))
    assert g.setSubmapKeyframes([0, 1, 2])
    a = g.voxelMap()
    pts, covs = g.targetPoints(), g.getTargetCovariances()
    assert len(pts) == sum(len(s) for s in scans)
    h = _map_engine(ng, pts, covs, 1.0)
    b = h.voxelMap()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    _check_map(a, vm.VoxelMap(pts, covs, 1.0), "submap")
    assert g.setSubmapKeyframes([0, 2])  # a new submap: a new map
    pts2 = g.targetPoints()
    assert g.voxelMap()[3].sum() == len(pts2) < len(pts)
    prod.close(); g.close(); h.close()


# ---- linearize / compute_error ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s2m(ng):
    """3k -> 6k (two keyframes), the engine's own covariances (k = 20), shared by the tests below and left unchanged."""
    w = clouds.scan_to_submap(3008, 2)
    g = ng.NanoGICP()
    g.setInputSource(w.source); g.setInputTarget(w.target)
    g.calculateSourceCovariances(); g.calculateTargetCovariances()
    cs, ct = g.getSourceCovariances(), g.getTargetCovariances()
    g.close()
    return dict(w=w, cs=cs, ct=ct, maps={})


def _engine(ng, src, tgt, cs, ct, res, **settings):
    g = ng.NanoGICP()
    g.setVoxelResolution(res)
    for name, v in settings.items():
        getattr(g, name)(v)
    g.setInputSource(src); g.setInputTarget(tgt)
    g.setSourceCovariances(cs); g.setTargetCovariances(ct)
    return g


def _model(s2m, src, cs, res, ct=None, tag=None, **kw):
    """The model on the shared target; its voxel map is built once per resolution (and per set of target covariances) and shared."""
    ct = s2m["ct"] if ct is None else ct
    m = vm.VoxelGICPModel.__new__(vm.VoxelGICPModel)
    vm.NumpyGICP.__init__(m, src, s2m["w"].target, cs, ct, **kw)
    if (res, tag) not in s2m["maps"]:
        s2m["maps"][res, tag] = vm.VoxelMap(m.tgt, ct, res)
    m.vmap = s2m["maps"][res, tag]
    return m


def _half_the_voxels_negative(s2m, res, seed=11):
    """The shared target covariances with those of every point in about half of the voxels replaced by -2 I (setTargetCovariances
    takes any matrix).  cov_v + R C_a R^T is then negative definite in those voxels, with eigenvalues in [-2, -1] (C_a's are 1e-3, 1, 1):
    as well conditioned as in the others, so the tolerances of the other cases hold, but the sum of squares is no longer one, a
    Gauss-Newton step from a poor guess goes uphill, and LM rejects trials until lambda has grown.  (No symmetric positive definite
    set that rejects a trial in this mode is known: under frozen voxels the error is quadratic in the translation.)"""
    ijk = vm.voxel_of(s2m["w"].target, res)
    key = ijk[:, 0] + 4096 * (ijk[:, 1] + 4096 * ijk[:, 2])
    uk = np.unique(key)
    neg = uk[np.random.default_rng(seed).random(len(uk)) < 0.5]
    ct = s2m["ct"].copy()
    ct[np.isin(key, neg), :3, :3] = -2.0 * np.eye(3)
    return ct


def _close(a, b, tol, what):
    scale = np.abs(b).max()
    d = np.abs(np.asarray(a) - np.asarray(b)).max()
    print(f"{what}: off by {d / scale if scale else d:.2e} of the largest entry")
    assert d <= tol * scale, what


@pytest.mark.parametrize("n_src,res", [(1, 1.0), (257, 0.25), (3008, 1.0), (3008, 4.0)])
def test_linearize_and_compute_error_match_the_model(ng, s2m, n_src, res):
    """H, b and err within 1e-9 of their largest entry (the project's bar for H and b); voxel numbers and float distances exact.
    The source carries points outside every voxel: far away, above the room, and (at 0.25 m) beyond 2^20 voxels."""
    w = s2m["w"]
    pick = np.linspace(0, 3007, n_src).astype(int) if n_src < 3008 else np.arange(3008)
    extra = np.array([[500, 500, 500], [3e5, 0, 0], [0.3, 0.2, 40.0]], np.float32)  # (3e5 m / 0.25 m > 2^20)
    src = np.ascontiguousarray(np.r_[w.source[pick], extra])
    cs = np.r_[s2m["cs"][pick], _spd(len(extra), 60)]
    g = _engine(ng, src, w.target, cs, s2m["ct"], res)
    m = _model(s2m, src, cs, res)
    for T in (_f32_pose(*[(0.3, 0.1, 0.02), (0.5, -0.3, 2.0)]), np.eye(4), _f32_pose((0.8, -0.5, 0.1), (1, -2, 6))):
        H, b, err = g.linearize(T)
        Hm, bm, em = m.linearize(T)
        corr, sqd = g.correspondences()
        assert np.array_equal(corr, m.corr), f"voxel numbers differ at {np.flatnonzero(corr != m.corr)[:5]}"
        assert (corr[-3:] == -1).all() and (n_src == 1 or (corr[:-3] >= 0).any())
        assert np.array_equal(sqd, m.sqd)
        _close(H, Hm, 1e-9, "H"); _close(b, bm, 1e-9, "b"); _close([err], [em], 1e-9, "err")
        assert np.array_equal(H, H.T)
        T2 = _f32_pose((0.01, -0.02, 0.005), (0.1, 0.05, -0.2)) @ T
        T2 = T2.astype(np.float32).astype(np.float64)
        _close([g.compute_error(T2)], [m.compute_error(T2)], 1e-9, "compute_error")
    g.close()


def test_a_source_outside_the_map_behaves_as_exact_gicp_without_correspondences(ng, s2m):
    """Pinned from the exact path first: align() when nothing passes the gate (the set-up of test_gpu_parity.test_zero_correspondences)."""
    w = s2m["w"]
    src = np.ascontiguousarray(w.source[:500])

    def outcome(g):
        g.align()
        return (g.getFinalTransformation().copy(), g.converged_, g.nr_iterations_, g.getFinalHessian().copy(), g.lm_trace().copy())

    ex = ng.NanoGICP()
    ex.setMaxCorrespondenceDistance(1e-6)
    ex.setInputSource(src); ex.setInputTarget(w.target[:500] + np.float32(80))
    want = outcome(ex)
    g = _engine(ng, src + np.float32(300), w.target, s2m["cs"][:500], s2m["ct"], 1.0)
    H, b, err = g.linearize(np.eye(4))
    assert not H.any() and not b.any() and err == 0.0 and (g.correspondences()[0] == -1).all()
    got = outcome(g)
    for a, e in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(e), equal_nan=True)
    ex.close(); g.close()


# ---- whole alignments, pass by pass ------------------------------------------------------------------------------------------------
_POOR_GUESS = clouds.make_pose((1.5, -1.0, 0.2), (2, -3, 12)).astype(np.float32)
ALIGN_CASES = {  # settings, guess (None: the workload's), resolution, target covariances (None: the shared ones)
    "lm_defaults": (dict(), None, 1.0, None),
    "gauss_newton": (dict(setOptimizer=0, setMaximumIterations=15), None, 1.0, None),
    "one_iteration": (dict(setMaximumIterations=1), None, 1.0, None),
    # the suite's LM-rejection configuration (_pass_check.CASES["lm_rejection"]: a poor guess and a vanishing initial lambda) on target
    # covariances under which this mode does reject: trials are rejected, then one is accepted, and again in a later iteration
    "lm_rejection": (dict(setMaximumIterations=12, setInitialLambdaFactor=1e-15), _POOR_GUESS, 1.0, "half_negative"),
    # the same with too few trials for lambda to grow: the alignment ends on a rejected trial
    "lm_rejection_to_the_end": (dict(setMaximumIterations=12, setInitialLambdaFactor=1e-15, setLMMaxIterations=4), _POOR_GUESS, 1.0, "half_negative"),
    "res_025": (dict(setMaximumIterations=6), None, 0.25, None),
}


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@pytest.mark.parametrize("case", sorted(ALIGN_CASES))
def test_every_pass_of_an_alignment_matches_the_model(ng, s2m, case):
    """tests/_pass_check.py's method with the model for the oracle: align(max_iter = m) for every m up to the full run; at the pose of
    every trace row's linearisation (the float pose the run of m - 1 iterations returned) the voxel numbers are exact, y0 / yi / H are
    within H_TOL (1e-5: the engine evaluates at its double pose, the model at double(float(pose))).  The run is repeated on a fresh
    handle: bit-identical.
    The lm_rejection cases must reject trials (asserted).  A rejected trial leaves the pose, the correspondences and the matrices of the
    linearisation in place for the next error pass; what pins that is yi of the trial accepted after rejected ones (it is computed from
    those buffers, and compared with the model's error under the model's frozen linearisation), y0 and the voxel numbers of the
    iteration that follows, and, where the run ends on a rejected trial, the unmoved pose and the Hessian of the last accepted step."""
    settings, guess, res, ct_tag = ALIGN_CASES[case]
    settings = dict(settings)
    w = s2m["w"]
    ct = _half_the_voxels_negative(s2m, res) if ct_tag else s2m["ct"]
    guess = np.asarray(w.guess if guess is None else guess, np.float32)
    max_iter = settings.pop("setMaximumIterations", 64)
    gn = settings.get("setOptimizer", 1) == 0
    g = _engine(ng, w.source, w.target, s2m["cs"], ct, res, **settings)
    m = _model(s2m, w.source, s2m["cs"], res, ct=ct, tag=ct_tag)
    g.setMaximumIterations(max_iter)
    g.align(guess)
    full = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), g.nr_iterations_, g.converged_)
    n_full = g.nr_iterations_ + 1
    start, end = clouds.pose_error(guess, w.gt), clouds.pose_error(full[0], w.gt)
    print(f"{case}: {n_full} iterations, converged {g.converged_}, {int((full[1][:, 7] == 0).sum()) if len(full[1]) else 0} rejected trials, "
          f"pose error {start[0]:.4f} m / {start[1]:.5f} rad -> {end[0]:.4f} m / {end[1]:.5f} rad")
    if case.startswith("lm_rejection"):  # the case is about rejected trials: it must have them
        acc, it = full[1][:, 7], full[1][:, 0]
        assert (acc == 0).any(), f"{case}: no trial was rejected"
        if case == "lm_rejection":  # rejected, then accepted; and rejected again after an accepted step has swapped the correspondence buffers
            assert (acc == 1).any() and ((acc == 0) & (it > 0)).any(), f"{case}: accepted {acc.astype(int).tolist()} in iterations {it.astype(int).tolist()}"
        else:
            assert acc[-1] == 0 and not g.converged_, f"{case}: accepted {acc.astype(int).tolist()}"
    poses, H_at = [guess], {}
    for k in range(1, n_full + 1):
        where = f"{case}: pass {k} of {n_full}"
        g.setMaximumIterations(k)
        g.align(guess)
        T, Hg, tr = g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.lm_trace().copy()
        corr, sqd = g.correspondences()
        P = poses[k - 1].astype(np.float64)
        Hm, _, em = m.linearize(P)
        assert np.array_equal(corr, m.corr), f"{where}: voxel numbers differ at queries {np.flatnonzero(corr != m.corr)[:5]}"
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
        print(f"{where}: gated in {(corr >= 0).mean():.4f}, |dH|/|H| {dH:.1e}, y0/yi rel. {dE:.1e}")
        assert dH <= H_TOL, f"{where}: |dH|/|H| = {dH:.2e}"
        n_rows = int(np.sum(full[1][:, 0] < k)) if len(full[1]) else 0
        assert tr.shape == (n_rows, 8) and np.array_equal(tr, full[1][:n_rows]), f"{where}: the LM trace is not a prefix of the full run's"
        poses.append(T)
    assert np.array_equal(poses[-1], full[0]) and np.array_equal(Hg, full[2]) and (g.nr_iterations_, g.converged_) == full[3:]
    # twice: bit-identical, on this handle and on a fresh one
    f = _engine(ng, w.source, w.target, s2m["cs"], ct, res, **settings)
    for e in (g, f):
        e.setMaximumIterations(max_iter)
        e.align(guess)
        assert np.array_equal(e.getFinalTransformation(), full[0]) and np.array_equal(e.lm_trace(), full[1]) and np.array_equal(e.getFinalHessian(), full[2])
        assert (e.nr_iterations_, e.converged_) == full[3:]
    if case == "lm_defaults":
        assert end[0] < start[0] and end[1] < start[1]
    g.close(); f.close()


# ---- mode hygiene ----------------------------------------------------------------------------------------------------------------
def test_switching_the_mode_off_restores_exact_gicp_bit_for_bit(ng, s2m):
    w = s2m["w"]

    def exact():
        e = ng.NanoGICP()
        e.setMaxCorrespondenceDistance(w.max_corr_dist)
        e.setInputSource(w.source); e.setInputTarget(w.target)
        e.setSourceCovariances(s2m["cs"]); e.setTargetCovariances(s2m["ct"])
        return e

    ref = exact()
    ref.align(w.guess)
    want = (ref.getFinalTransformation().copy(), ref.lm_trace().copy(), ref.getFinalHessian().copy(), ref.correspondences())
    g = exact()
    g.setVoxelResolution(1.0)
    g.align(w.guess)
    T_vox = g.getFinalTransformation().copy()
    assert g.correspondences()[0].max() < g.getVoxelMapSize()
    g.setVoxelResolution(0)
    with pytest.raises(ng.NgicpError):  # the voxel numbers of the other mode are not target indices
        g.correspondences()
    g.align(w.guess)
    assert np.array_equal(g.getFinalTransformation(), want[0]) and np.array_equal(g.lm_trace(), want[1]) and np.array_equal(g.getFinalHessian(), want[2])
    c = g.correspondences()
    assert np.array_equal(c[0], want[3][0]) and np.array_equal(c[1], want[3][1])
    assert not np.array_equal(T_vox, want[0])  # a different algorithm: a different answer
    ref.close(); g.close()


def test_correspondences_go_with_the_map_they_number(ng, s2m):
    """Voxel numbers index one map's records: once the target or its covariances change, they are no longer handed out (and
    compute_error asks for a new linearize), also after the next map has been built."""
    w = s2m["w"]
    g = _engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0)
    g.align(w.guess)
    assert (g.correspondences()[0] >= 0).any()
    g.setInputTarget(np.ascontiguousarray(w.target[::2]))
    g.voxelMap()
    with pytest.raises(ng.NgicpError):
        g.correspondences()
    g.linearize(np.eye(4))
    g.correspondences()
    g.setTargetCovariances(_spd(len(w.target[::2]), 70))
    with pytest.raises(ng.NgicpError):
        g.compute_error(np.eye(4))
    with pytest.raises(ng.NgicpError):
        g.correspondences()
    g.close()


def test_max_correspondence_distance_is_not_consulted(ng, s2m):
    w = s2m["w"]
    a = _engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0)
    b = _engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, setMaxCorrespondenceDistance=1e-3)
    a.align(w.guess); b.align(w.guess)
    assert np.array_equal(a.getFinalTransformation(), b.getFinalTransformation()) and np.array_equal(a.lm_trace(), b.lm_trace())
    a.close(); b.close()


def test_batch_and_sharded_entries_are_refused_while_the_mode_is_on(ng, s2m):
    w = s2m["w"]
    g = _engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0)
    calls = [lambda: g.alignBatch(np.repeat(np.eye(4, dtype=np.float32)[None], 2, 0)), lambda: g.sharded_begin(), lambda: g.sharded_pass(0),
             lambda: g.sharded_step(0), lambda: g.sharded_finish(), lambda: g.covsShardBegin(1), lambda: g.covsShardCompute(1, 0, 1), lambda: g.covsShardCommit(1)]
    for call in calls:
        with pytest.raises(ng.NgicpError) as e:
            call()
        assert e.value.code == -2 and "not available with a voxelized target" in str(e.value)
    # the queries are unaffected
    idx, _ = g.nearestKSearch(w.target[:5], 1)
    assert idx[:, 0].tolist() == [0, 1, 2, 3, 4]
    assert g.fitness()[1] == len(w.source)
    g.setVoxelResolution(0)
    T, _, _, _ = g.alignBatch(np.repeat(np.asarray(w.guess, np.float32)[None], 2, 0))
    assert np.array_equal(T[0], T[1])
    g.close()
