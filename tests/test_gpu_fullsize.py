"""Full-size HIP-vs-oracle parity (-m gpu) on every single-GPU configuration of BASELINE.json:
  c2  scan-to-scan 100k vs 100k VLP-16-shaped (gate 1.0 m and the unbounded default)
  c3  scan-to-submap 100k vs 500k (5 keyframes), DLO's settings (32 / 0.01 / 2e-3) and the bench's fixed 20 iterations
  c5  dense OS1-128-shaped 250k vs 2M (8 keyframes)
(c4 is c3 once per GPU.)  Each case compares, on SHARED covariances (the GPU's, checked against the oracle's away from k-NN
boundary ties first): the linearisation at the initial guess (correspondences, float32 squared distances, H, b, error), the
alignment (final transform <= 1e-4 m / 1e-4 rad per BASELINE.json north_star, nr_iterations, converged, accept/reject sequence),
and the correspondences at the final pose.  Correspondence indices must agree wherever the nearest neighbour is unique; where
two target points are EXACTLY equidistant in float32 the reference keeps whichever its kd-tree visits first
(impl/nanoflann_impl.hpp:184-211, SURVEY.md §7 "Ties"), so there the squared distances must still agree bit for bit."""
import numpy as np
import pytest

from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

DLO = dict(setMaximumIterations=32, setTransformationEpsilon=0.01)                                   # cfg/params.yaml:57-60,66-69
FIXED20 = dict(setMaximumIterations=20, setTransformationEpsilon=1e-12, setRotationEpsilon=1e-12)    # SURVEY.md §8d "20 GICP iters"


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _ties(orc, pts, k, threads=16):
    _, d2 = orc.OracleTree(pts).knn(pts, k + 1, threads)
    return d2[:, k - 1] == d2[:, k]


def _check_covs(orc, pts, sizes, k, gpu_covs):
    """GPU covariances vs the oracle's, keyframe by keyframe, away from k-NN boundary ties."""
    lo = 0
    for n in sizes:
        kf = np.ascontiguousarray(pts[lo:lo + n])
        ref = orc.covariances(kf, k, 3, 16)
        ties = _ties(orc, kf, k)
        assert ties.mean() < 2e-3
        assert np.abs(gpu_covs[lo:lo + n] - ref)[~ties].max() < 1e-9
        lo += n


def _point_terms(src, tgt, cs, ct, rows, corr, T):
    """Sum over `rows` of the per-point terms of H, b and the error (impl/nano_gicp_impl.hpp:205-209,232-257) in float64 numpy."""
    H, b, err = np.zeros((6, 6)), np.zeros(6), 0.0
    R, t = T[:3, :3], T[:3, 3]
    for i, j in zip(rows, corr):
        M = np.linalg.inv(ct[j][:3, :3] + R @ cs[i][:3, :3] @ R.T)
        ta = R @ src[i].astype(np.float64) + t
        e = tgt[j].astype(np.float64) - ta
        J = np.hstack([np.array([[0, -ta[2], ta[1]], [ta[2], 0, -ta[0]], [-ta[1], ta[0], 0.0]]), -np.eye(3)])
        H += J.T @ M @ J
        b += J.T @ M @ e
        err += e @ M @ e
    return H, b, err


def _compare_linearisation(g, o, T, src, tgt, cs, ct):
    Hg, bg, eg = g.linearize(T)
    Ho, bo, eo = o.linearize(T)
    cg, sg = g.correspondences(); co, so = o.correspondences()
    assert np.array_equal(cg >= 0, co >= 0)                      # the same points pass the distance gate
    assert np.array_equal(sg[cg >= 0], so[co >= 0])              # float32 squared distances, bit for bit
    differ = np.flatnonzero(cg != co)
    assert len(differ) < 1e-3 * len(cg)                          # only exact-distance ties may pick another index (checked above: equal d2)
    if len(differ):
        # A tie resolved the other way swaps one target point (and its covariance) for an equidistant one.  The tolerance is NOT
        # widened for that: the oracle's sums are re-based onto the GPU's correspondences for exactly those rows (their terms under
        # the oracle's choice taken out, under the GPU's choice put in), and the comparison stays at 1e-9.
        Hm, bm, em = _point_terms(src, tgt, cs, ct, differ, co[differ], T)
        Hp, bp, ep = _point_terms(src, tgt, cs, ct, differ, cg[differ], T)
        Ho, bo, eo = Ho - Hm + Hp, bo - bm + bp, eo - em + ep
    print(f"linearisation: {len(differ)} correspondences differ on exact float32 distance ties; |dH|/|H| = {np.abs(Hg - Ho).max() / np.abs(Ho).max():.2e}")
    tol = 1e-9
    assert abs(eg - eo) <= tol * abs(eo)
    assert np.abs(Hg - Ho).max() <= tol * np.abs(Ho).max() and np.abs(bg - bo).max() <= tol * np.abs(bo).max(), (len(differ), np.abs(Hg - Ho).max() / np.abs(Ho).max())
    return len(differ)


def _check_last_pass(g, o, guess, tg, src, tgt, cs, ct):
    """g has just aligned from `guess`: its correspondences are those of the pass at the float pose x0 had when the last iteration began -
    the returned pose itself when the alignment ended on rejected trials, else the pose one iteration shorter alignment returns."""
    # (the per-pass check lives in tests/_pass_check.py, shared with test_gpu_passes.py, the module that documents it; pytest puts
    # tests/ on sys.path)
    from _pass_check import check_pass
    cg, sg = g.correspondences()
    n, T = g.nr_iterations_ + 1, g.getFinalTransformation().copy()
    if len(tg) and tg[-1, 7] == 0:
        P = T
    elif n == 1:
        P = np.asarray(guess, np.float32)
    else:
        max_iter = g._p["max_iter"]
        g.setMaximumIterations(n - 1)
        g.align(guess)
        P = g.getFinalTransformation().copy()
        g.setMaximumIterations(max_iter)
    return check_pass(f"last pass ({n})", P, cg, sg, o, src, tgt, cs, ct)["ties"]


def _run_case(ng, orc, w, k, gate, settings, guess, tgt_sizes=None):
    g, o = ng.NanoGICP(), orc.OracleGICP()
    o.setNumThreads(16)
    for e in (g, o):
        e.setCorrespondenceRandomness(k)
        if gate is not None:
            e.setMaxCorrespondenceDistance(gate)
        for name, v in settings.items():
            getattr(e, name)(v)
        e.setInputSource(w.source); e.setInputTarget(w.target)
    # covariances: the GPU's, verified against the oracle's, shared with it
    g.calculateSourceCovariances()
    cs = g.getSourceCovariances()
    _check_covs(orc, w.source, [len(w.source)], k, cs)
    if tgt_sizes is None:
        g.calculateTargetCovariances()
        ct = g.getTargetCovariances()
        _check_covs(orc, w.target, [len(w.target)], k, ct)
    else:  # per-keyframe covariances, concatenated (odom.cc:1172-1174,1318-1325), supplied as DLO does (odom.cc:833)
        ct = ng.keyframe_covariances(w.target, tgt_sizes, k)
        _check_covs(orc, w.target, tgt_sizes, k, ct)
        g.setTargetCovariances(ct)
    o.setSourceCovariances(cs); o.setTargetCovariances(ct)
    n_tie0 = _compare_linearisation(g, o, np.asarray(guess, np.float64), w.source, w.target, cs, ct)
    g.align(guess); o.align(guess)
    s, iters = g.stats(), g.nr_iterations_
    Tg, To = g.getFinalTransformation(), o.getFinalTransformation()
    dt, dr = clouds.pose_error(Tg, To)
    assert dt <= 1e-4 and dr <= 1e-4, (dt, dr)
    tg, to = g.lm_trace(), o.lm_trace()
    if settings is FIXED20:
        # eps = 1e-12: the loop ends on max_iterations or when LM gives up at the noise floor (rho ~ 0/0); which iteration that
        # happens in is rounding noise, so only the common prefix of the trace is comparable (as in test_gpu_parity.py)
        m = min(len(tg), len(to), 4)
        assert np.array_equal(tg[:m, [0, 1, 7]], to[:m, [0, 1, 7]]) and np.allclose(tg[:m, 2:4], to[:m, 2:4], rtol=1e-6)
    else:
        assert g.nr_iterations_ == o.nr_iterations and g.converged_ == o.converged
        assert tg.shape == to.shape and np.array_equal(tg[:, [0, 1, 7]], to[:, [0, 1, 7]])
        assert np.allclose(tg[:, 2:4], to[:, 2:4], rtol=1e-6)
        cg, _ = g.correspondences(); co, _ = o.correspondences()    # correspondences_ after align(): the last linearisation's
        assert np.array_equal(cg >= 0, co >= 0) and (cg != co).mean() < 1e-3
    # The correspondences align() leaves behind are those of its last adopted linearisation, a WARM pass: checked exactly against a cold
    # oracle search at the GPU's own float pose of that pass (test_gpu_passes.py's per-pass check), with either settings
    n_tie_last = _check_last_pass(g, o, guess, tg, w.source, w.target, cs, ct)
    n_tie1 = _compare_linearisation(g, o, Tg.astype(np.float64), w.source, w.target, cs, ct)   # and at the final pose, distances bit for bit
    return dict(dt=dt, dr=dr, ties=(n_tie0, n_tie_last, n_tie1), iters=iters, cand=s["mean_candidates"])


@pytest.mark.parametrize("gate", [1.0, None])
def test_c2_scan_to_scan_100k(ng, oracle_mod, gate):
    w = clouds.scan_to_scan(100_000)
    r = _run_case(ng, oracle_mod, w, 10 if gate else 20, gate, DLO if gate else {}, w.guess)
    print("c2", gate, r)


@pytest.mark.parametrize("settings", [DLO, FIXED20], ids=["dlo", "fixed20"])
def test_c3_scan_to_submap_100k_500k(ng, oracle_mod, settings):
    w = clouds.scan_to_submap(100_000, 5)
    r = _run_case(ng, oracle_mod, w, 20, w.max_corr_dist, settings, w.guess, w.keyframe_sizes)
    print("c3", r)


@pytest.mark.parametrize("settings", [DLO, FIXED20], ids=["dlo", "fixed20"])
def test_c5_dense_os1_250k_2m(ng, oracle_mod, settings):
    w = clouds.scan_to_submap(250_000, 8, shape="os1")
    assert len(w.source) == 250_000 and len(w.target) == 2_000_000
    r = _run_case(ng, oracle_mod, w, 20, w.max_corr_dist, settings, w.guess, w.keyframe_sizes)
    print("c5", r)


@pytest.mark.parametrize("g_rank", [1, 2, 3, 4, 5, 6, 7])
def test_c4_seed_offset_workloads_on_one_gpu(ng, oracle_mod, g_rank):
    """BASELINE configs[3] is one c3-shaped alignment per GPU with seeds offset by 1000 * g (bench.py build_workload); rank 0 is the
    c3 case above.  No 8-GPU lease exists for the builder, but the seven other WORKLOADS run here, one after the other on one GPU,
    through the same checks."""
    w = clouds.scan_to_submap(100_000, 5, seed_offset=1000 * g_rank)
    r = _run_case(ng, oracle_mod, w, 20, w.max_corr_dist, FIXED20, w.guess, w.keyframe_sizes)
    print("c4 rank", g_rank, r)


def test_source_larger_than_the_sorted_launch_list(ng, oracle_mod):
    """A 500k-point SOURCE (the submap aligned back onto the scan): more groups of query batches than the solver sorts into a launch
    list (kMaxOrderGroups = 4096), so the pass runs in index order and the solver reduces its rows in several steps - the largest
    grid any configuration launches.  Same checks as the BASELINE configurations."""
    from types import SimpleNamespace
    w = clouds.scan_to_submap(100_000, 5)
    inv = np.linalg.inv(np.asarray(w.guess, np.float64)).astype(np.float32)
    sw = SimpleNamespace(source=w.target, target=w.source)
    r = _run_case(ng, oracle_mod, sw, 10, 1.0, DLO, inv)
    print("500k source", r)
