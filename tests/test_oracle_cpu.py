"""CPU tests: the oracle against the reference's real kd-tree (golden vectors + live when available),
against the independent numpy model, and its small linear-algebra pieces against LAPACK/scipy.
The reference ships no tests of its own; paths cited are under /root/reference/include/nano_gicp/."""
import os

import numpy as np
import pytest

from direct_lidar_odometry_amd import clouds
from oracle import numpy_model as nm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_oracle_kdtree_matches_reference_golden(golden, oracle_mod):
    """Golden kNN vectors were produced by the REAL reference nanoflann (tests/golden/make_golden.py)."""
    src, tgt, probes = golden["source"], golden["target"], golden["probes"]
    t = oracle_mod.OracleTree(tgt)
    for k, name in ((1, "ref_knn1"), (20, "ref_knn20")):
        idx, d2 = t.knn(src[probes], k)
        assert np.array_equal(idx, golden[name + "_idx"])
        assert np.array_equal(d2, golden[name + "_d2"])  # bit-exact float32
    ts = oracle_mod.OracleTree(src)
    idx, d2 = ts.knn(src[probes], 20)
    assert np.array_equal(idx, golden["ref_selfknn20_idx"]) and np.array_equal(d2, golden["ref_selfknn20_d2"])
    assert np.all(d2[:, 0] == 0.0) and np.array_equal(idx[:, 0], probes)  # self is its own nearest neighbour


@pytest.fixture(scope="module")
def ref_kdtree():
    """The reference kd-tree's outputs on stored inputs (tests/golden/make_ref_kdtree.py)."""
    with np.load(os.path.join(GOLDEN, "ref_kdtree.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _check_against_reference(oracle_mod, ref_kdtree, key, k):
    pts, q = ref_kdtree[key + "_pts"], ref_kdtree[key + "_q"]
    want_idx, want_d2 = ref_kdtree[key + "_idx"], ref_kdtree[key + "_d2"]
    assert want_idx.shape == (len(q), k)
    a = oracle_mod.OracleTree(pts).knn(q, k)
    assert np.array_equal(a[1], want_d2) and np.array_equal(a[0], want_idx)
    if oracle_mod.ref_available():  # where oracle/_ref is built, the live reference must still give the stored answer
        b = oracle_mod.RefTree(pts).knn(q, k)
        assert np.array_equal(b[1], want_d2) and np.array_equal(b[0], want_idx)


@pytest.mark.parametrize("n,k", [(1, 1), (7, 3), (101, 20), (100, 20), (5000, 1), (5000, 20), (20000, 32)])
def test_oracle_kdtree_matches_reference_live(oracle_mod, ref_kdtree, n, k):
    """Index-for-index against the reference kd-tree on seeded normal clouds (queries inside and far outside): the reference's
    answers are stored with their inputs in tests/golden/ref_kdtree.npz."""
    assert len(ref_kdtree[f"n{n}_k{k}_pts"]) == n
    _check_against_reference(oracle_mod, ref_kdtree, f"n{n}_k{k}", min(k, n))


def test_oracle_kdtree_ties_and_duplicates(oracle_mod, ref_kdtree):
    """Exact ties: traversal order decides (impl/nanoflann_impl.hpp:184-211); the restatement must agree with the reference."""
    _check_against_reference(oracle_mod, ref_kdtree, "ties", 8)


def test_oracle_knn_vs_bruteforce(oracle_mod, golden):
    tgt, src = golden["target"], golden["source"]
    idx, d2 = oracle_mod.OracleTree(tgt).knn(src[:300], 20)
    bi, bd = nm.knn_bruteforce(src[:300], tgt, 20)
    assert np.array_equal(d2, bd)
    assert np.mean(idx == bi) > 0.999  # indices may differ only where distances tie exactly


def test_oracle_small_linear_algebra(oracle_mod):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    for scale in (1e-7, 1e-3, 0.3, 2.5):
        w = rng.normal(size=3) * scale
        assert np.abs(oracle_mod.so3_exp(w) - Rotation.from_rotvec(w).as_matrix()).max() < 1e-14
    assert np.abs(oracle_mod.so3_exp(np.zeros(3)) - np.eye(3)).max() == 0.0
    for _ in range(20):
        A = rng.normal(size=(6, 6)); A = A @ A.T + 1e-3 * np.eye(6)
        rhs = rng.normal(size=6)
        assert np.abs(oracle_mod.ldlt6_solve(A, rhs) - np.linalg.solve(A, rhs)).max() < 1e-9 * np.abs(np.linalg.solve(A, rhs)).max()
    assert np.all(oracle_mod.ldlt6_solve(np.zeros((6, 6)), np.zeros(6)) == 0.0)  # Eigen's LDLT returns 0 for the zero system
    for _ in range(20):
        B = rng.normal(size=(3, 3)); B = B @ B.T
        w, V = oracle_mod.eig3_sym(B)
        assert np.all(np.diff(w) <= 0)
        assert np.abs(V @ np.diag(w) @ V.T - B).max() < 1e-12 * np.abs(B).max()
        assert np.abs(np.sort(w) - np.linalg.eigvalsh(B)).max() < 1e-12 * np.abs(B).max()


@pytest.mark.parametrize("reg,name", [(0, "NONE"), (1, "MIN_EIG"), (2, "NORMALIZED_MIN_EIG"), (3, "PLANE"), (4, "FROBENIUS")])
def test_oracle_covariances_vs_numpy_svd(oracle_mod, golden, reg, name):
    """All five RegularizationMethod branches (impl/nano_gicp_impl.hpp:323-353) against a real SVD."""
    pts = golden["source"][:400]
    a = oracle_mod.covariances(pts, k=20, reg=reg)
    b = nm.covariances(pts, k=20, reg=name)
    assert np.abs(a - b).max() < 1e-9
    assert np.all(a[:, 3, :] == 0) and np.all(a[:, :, 3] == 0)


def test_oracle_k_larger_than_cloud_is_an_error(oracle_mod):
    pts = np.random.default_rng(1).normal(size=(10, 3)).astype(np.float32)
    with pytest.raises(RuntimeError):
        oracle_mod.covariances(pts, k=20)


def test_oracle_matches_golden_and_numpy_model(oracle_mod, golden):
    src, tgt = golden["source"], golden["target"]
    o = oracle_mod.OracleGICP()
    o.setMaxCorrespondenceDistance(float(golden["max_corr_dist"]))
    o.setInputSource(src); o.setInputTarget(tgt)
    o.calculateSourceCovariances(); o.calculateTargetCovariances()
    p = golden["probes"]
    assert np.abs(o.getSourceCovariances()[p] - golden["cov_src_probes"]).max() < 1e-12
    assert np.abs(o.getTargetCovariances()[p] - golden["cov_tgt_probes"]).max() < 1e-12
    H, b, err = o.linearize(golden["guess"].astype(np.float64))
    assert np.array_equal(o.correspondences()[0], golden["corr"])
    assert abs(err - float(golden["err"])) <= 1e-11 * abs(err)  # thread-order dependent summation
    assert np.abs(H - golden["H"]).max() <= 1e-11 * np.abs(H).max() and np.abs(b - golden["b"]).max() <= 1e-11 * np.abs(b).max()
    assert abs(o.compute_error(golden["T1"]) - float(golden["err_T1"])) <= 1e-11 * float(golden["err_T1"])
    T = o.align(golden["guess"])
    dt, dr = clouds.pose_error(T, golden["final_T"])
    assert dt < 1e-6 and dr < 1e-6
    assert o.nr_iterations == int(golden["nr_iterations"]) and o.converged == bool(golden["converged"])
    tr = o.lm_trace()
    assert tr.shape == golden["lm_trace"].shape and np.allclose(tr, golden["lm_trace"], rtol=1e-6, atol=1e-9)
    # independent numpy model on a 600-point subset (brute force, python loops)
    s2, t2 = src[::4], tgt[::4]
    cs, ct = nm.covariances(s2, 20), nm.covariances(t2, 20)
    o2 = oracle_mod.OracleGICP(); o2.setMaxCorrespondenceDistance(1.5)
    o2.setInputSource(s2); o2.setInputTarget(t2); o2.calculateSourceCovariances(); o2.calculateTargetCovariances()
    assert np.abs(o2.getSourceCovariances() - cs).max() < 1e-9
    m = nm.NumpyGICP(s2, t2, cs, ct, max_corr_dist=1.5)
    Tn = m.align(np.eye(4)); To = o2.align(np.eye(4))
    dt, dr = clouds.pose_error(Tn, To)
    assert dt < 1e-6 and dr < 1e-6 and m.nr_iterations == o2.nr_iterations and m.converged == o2.converged


def test_oracle_call_sequence_semantics(oracle_mod, golden):
    """Pointer-identity early-out, swap and covariance caching (impl/nano_gicp_impl.hpp:91-98,113-139,162-171)."""
    src, tgt = golden["source"], golden["target"]
    o = oracle_mod.OracleGICP(); o.setMaxCorrespondenceDistance(1.0)
    o.setInputSource(src); o.setInputTarget(tgt)
    T_fwd = o.align()
    ns, nt = len(o.getSourceCovariances()), len(o.getTargetCovariances())
    assert ns == len(src) and nt == len(tgt)  # computed lazily inside align
    o.setInputSource(src)  # same identity: covariances survive
    assert len(o.getSourceCovariances()) == ns
    o.swapSourceAndTarget()
    T_bwd = o.align()
    dt, dr = clouds.pose_error(np.linalg.inv(T_bwd.astype(np.float64)), T_fwd)
    assert dt < 0.02 and dr < 0.01  # backward alignment is roughly the inverse
    o.setInputSource(src.copy())  # new identity: covariances cleared
    assert len(o.getSourceCovariances()) == 0


def test_oracle_zero_correspondences(oracle_mod, golden):
    """NaN rho is accepted and the identity step converges."""
    o = oracle_mod.OracleGICP(); o.setMaxCorrespondenceDistance(1e-6)
    o.setInputSource(golden["source"][:200]); o.setInputTarget(golden["target"][:200] + np.float32(50))
    T = o.align()
    assert np.array_equal(T, np.eye(4, dtype=np.float32)) and o.converged and o.nr_iterations == 0


@pytest.mark.parametrize("which", ["golden", "scan_to_scan_10k"])
def test_per_pass_method_on_the_oracle(oracle_mod, golden, which):
    """The method of test_gpu_passes.py, proven on the oracle alone: after align(max_iter=m), correspondences() are those of a cold
    linearize() at the float pose that align(max_iter=m-1) returned (P_0 = the guess) - index for index, distance for distance - and the
    trace is the first rows of the full run's.  So the GPU harness compares like with like."""
    if which == "golden":
        src, tgt, guess, gate = golden["source"], golden["target"], golden["guess"].astype(np.float32), float(golden["max_corr_dist"])
        settings = dict(max_iter=64)
    else:
        w = clouds.scan_to_scan(10_000)
        src, tgt, guess, gate = w.source, w.target, clouds.make_pose((0.3, -0.2, 0.05), (1.0, -1.0, 4.0)).astype(np.float32), 1.0
        settings = dict(max_iter=20, eps=1e-12)

    def handle():
        o = oracle_mod.OracleGICP()
        o.setNumThreads(1)  # (the oracle's OpenMP reduction order depends on the thread schedule: one thread makes the trace reproducible)
        o.setMaxCorrespondenceDistance(gate)
        if "eps" in settings:
            o.setTransformationEpsilon(settings["eps"]); o.setRotationEpsilon(settings["eps"])
        o.setInputSource(src); o.setInputTarget(tgt)
        return o

    a, b = handle(), handle()
    a.setMaximumIterations(settings["max_iter"])
    a.align(guess)
    full_tr, n_full = a.lm_trace(), a.nr_iterations + 1
    b.setSourceCovariances(a.getSourceCovariances()); b.setTargetCovariances(a.getTargetCovariances())
    assert n_full >= 3
    P = guess
    for m in range(1, n_full + 1):
        a.setMaximumIterations(m)
        a.align(guess)
        tr = a.lm_trace()
        k = int(np.sum(full_tr[:, 0] < m))
        assert tr.shape == (k, 8) and np.array_equal(tr, full_tr[:k]), m
        ca, sa = a.correspondences()
        b.linearize(P.astype(np.float64))
        cb, sb = b.correspondences()
        assert np.array_equal(ca, cb) and np.array_equal(sa, sb), m
        assert (ca >= 0).mean() > 0.5
        P = a.getFinalTransformation()
