"""Several initial guesses at once against a voxelized target on the GPU (ngicp_voxel_align_batch / alignBatchVoxel;
k_vgicp_pass_batch in csrc/ngicp_voxel_batch.h).

The yardstick is the single path, which test_gpu_vgicp.py and test_gpu_vgicp_nbr.py hold to the numpy model pass by pass: lane g of a
batch must be the same BITS as align(guesses[g]) on the same handle - transformation, convergence flag, iteration count, Hessian and LM
trace - under DIRECT1, DIRECT7 and DIRECT27.  One case per neighbourhood goes through the model directly as well.  Tolerances are the
project's (_pass_check.H_TOL for per-pass y0 / yi / H, voxel numbers exact); the selection recipe uses test_gpu_batch.py's bound."""
import threading

import numpy as np
import pytest

import _batch_cases as bc
import _vgicp_batch_cases as vbc
from _pass_check import H_TOL
from direct_lidar_odometry_amd import clouds
from test_gpu_batch import TOL_R, TOL_T
from test_gpu_vgicp import ALIGN_CASES, _POOR_GUESS, _engine, _f32_pose, _half_the_voxels_negative, _model, _rel, ng, s2m  # noqa: F401  (ng, s2m: fixtures)
from test_gpu_vgicp_nbr import _half_negative, _nbr_model

pytestmark = pytest.mark.gpu

KS = (1, 7, 27)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
    """np.array_equal on the raw bits: a NaN equals the same NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _guesses(w):
    """Nine guesses: the workload's, the identity, the poor guess of the LM-rejection cases, five poses from 5 cm to a few metres off the
    workload's guess, and one 500 m away, where no slot of any point has a voxel."""
    g0 = np.asarray(w.guess, np.float64)
    off = [((0.05, 0.0, 0.0), (0, 0, 0)), ((0.3, -0.2, 0.05), (0, 0, 5)), ((1.0, 0.5, 0.0), (1, -2, 20)), ((-2.0, 1.5, 0.2), (0, 0, 45)), ((3.0, -2.5, 0.3), (3, 2, 90))]
    out = [g0, np.eye(4), _POOR_GUESS] + [g0 @ clouds.make_pose(t, r) for t, r in off] + [clouds.make_pose((500, 500, 500))]
    return np.ascontiguousarray(np.stack([np.asarray(x, np.float32) for x in out]))


def _kengine(ng, src, tgt, cs, ct, res, K, **settings):
    g = _engine(ng, src, tgt, cs, ct, res, **settings)
    g.setNeighborSearchMethod(K)
    return g


def _single(g, guesses):
    """align() per guess on handle g -> per guess (T, converged, iterations, H, trace)."""
    out = []
    for q in guesses:
        g.align(q)
        out.append((g.getFinalTransformation().copy(), bool(g.hasConverged()), int(g.nr_iterations_), g.getFinalHessian().copy(), g.lm_trace().copy()))
    return out


def _assert_lanes_equal(res, traces, refs, label=""):
    T, conv, its, H = res
    assert T.shape == (len(refs), 4, 4) and T.dtype == np.float32 and H.shape == (len(refs), 6, 6) and H.dtype == np.float64
    for lane, (rT, rconv, rits, rH, rtrace) in enumerate(refs):
        where = f"{label} lane {lane}"
        assert _same_bits(T[lane], rT), where
        assert bool(conv[lane]) == rconv and int(its[lane]) == rits, (where, conv[lane], its[lane], rconv, rits)
        assert _same_bits(H[lane], rH), where
        assert traces[lane].shape == rtrace.shape and _same_bits(traces[lane], rtrace), where


def _batch_then_singles(g, G, label):
    """alignBatchVoxel(G) on g, then align(G[i]) for every i on the SAME handle: every lane bit for bit.  -> (batch result, traces)."""
    res = g.alignBatchVoxel(G)
    traces = [g.lm_trace(lane=i).copy() for i in range(len(G))]
    _assert_lanes_equal(res, traces, _single(g, G), label)
    return res, traces


# ---- 1. lane parity ---------------------------------------------------------------------------------------------------------------
PARITY_CASES = {  # settings, the target covariances' tag
    "lm_defaults": (dict(), None),
    "gauss_newton": (dict(setOptimizer=0, setMaximumIterations=15), None),
    "one_iteration": (dict(setMaximumIterations=1), None),
    "no_iterations": (dict(setMaximumIterations=0), None),
    "lm_rejection": (ALIGN_CASES["lm_rejection"][0], "half_negative"),
    "lm_rejection_to_the_end": (ALIGN_CASES["lm_rejection_to_the_end"][0], "half_negative"),
}


def _target_covs(s2m, res, K, tag):
    if not tag:
        return s2m["ct"]
    return _half_the_voxels_negative(s2m, res) if K == 1 else _half_negative(s2m, res, K)[0]  # (the draw each K's own test file uses)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", sorted(PARITY_CASES))
def test_lane_is_the_single_align_bit_for_bit(ng, s2m, case, K):
    settings, tag = PARITY_CASES[case]
    w = s2m["w"]
    G = _guesses(w)
    assert len(G) >= 8
    g = _kengine(ng, w.source, w.target, s2m["cs"], _target_covs(s2m, 1.0, K, tag), 1.0, K, **settings)
    (T, conv, its, H), traces = _batch_then_singles(g, G, f"{case} DIRECT{K}")
    rejected = [int((t[:, 7] == 0).sum()) if len(t) else 0 for t in traces]
    print(f"{case} DIRECT{K}: iterations {its.tolist()}, converged {conv.astype(int).tolist()}, rejected trials {rejected}")
    if settings.get("setMaximumIterations", 64) > 1:  # a lane really leaves the live list while others run
        assert len(set(its.tolist())) > 1, its.tolist()
    else:
        assert not its.any()
    if settings.get("setMaximumIterations", 64) == 0:
        assert np.array_equal(T, G) and not conv.any() and all(len(t) == 0 for t in traces)
    if tag:
        assert any(rejected), f"{case} DIRECT{K}: no lane rejected a trial"
    # the lane 500 m away matched nothing
    assert np.array_equal(T[-1], G[-1])
    g.close()


# ---- 2. shapes at which the grid can go wrong ---------------------------------------------------------------------------------------
def _small_source(s2m, n_src):
    """test_linearize_and_compute_error_match_the_model's sources: a partial block, an exact block, one point over, two blocks and one."""
    w = s2m["w"]
    pick = np.array([1500]) if n_src == 1 else np.linspace(0, 3007, n_src).astype(int)
    return np.ascontiguousarray(w.source[pick]), s2m["cs"][pick]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n_src", [1, 255, 256, 257, 513])
def test_block_edges(ng, s2m, n_src, K):
    w = s2m["w"]
    src, cs = _small_source(s2m, n_src)
    g = _kengine(ng, src, w.target, cs, s2m["ct"], 1.0, K)
    _batch_then_singles(g, _guesses(w)[[0, 3, 4, 8]], f"n_src {n_src} DIRECT{K}")
    g.close()


@pytest.mark.parametrize("K", KS)
def test_one_lane_and_sixty_four(ng, s2m, K):
    w = s2m["w"]
    g = _kengine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, K)
    _batch_then_singles(g, _guesses(w)[4:5], f"B = 1 DIRECT{K}")
    g.close()
    src, cs = _small_source(s2m, 257)
    g0 = np.asarray(w.guess, np.float64)
    G = np.stack([(g0 @ clouds.make_pose((0.02 * i, -0.01 * i, 0.001 * i), (0, 0, 0.5 * i))).astype(np.float32) for i in range(ng.BATCH_MAX_LANES)])
    assert len(np.unique(G.reshape(64, -1), axis=0)) == 64
    g = _kengine(ng, src, w.target, cs, s2m["ct"], 1.0, K)
    (_, _, its, _), _ = _batch_then_singles(g, G, f"B = 64 DIRECT{K}")
    print(f"B = 64 DIRECT{K}: iterations {its.tolist()}")
    g.close()


@pytest.mark.parametrize("K", KS)
def test_buffers_are_reused_and_regrown(ng, s2m, K):
    """B = 8, then B = 3, then - after a larger source - B = 8 again, on one handle."""
    w = s2m["w"]
    G = _guesses(w)
    src, cs = _small_source(s2m, 513)
    g = _kengine(ng, src, w.target, cs, s2m["ct"], 1.0, K)
    _batch_then_singles(g, G[:8], f"513 points, 8 lanes, DIRECT{K}")
    _batch_then_singles(g, G[5:8], f"513 points, 3 lanes, DIRECT{K}")
    g.setInputSource(w.source); g.setSourceCovariances(s2m["cs"])
    _batch_then_singles(g, G[:8], f"3008 points, 8 lanes, DIRECT{K}")
    g.close()


# ---- 3. held to the model directly --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_two_lanes_of_a_batch_match_the_model_pass_by_pass(ng, s2m, K):
    """_check_every_pass's method (test_gpu_vgicp_nbr.py) with the batch in align's place: alignBatchVoxel(max_iter = k) for every k up to
    the full run.  A lane's pose after k - 1 iterations is where iteration k - 1 linearises: there the model's error is the trace's y0,
    the model's error of the accepted trial its yi, and the model's H the lane's Hessian, all within H_TOL; after a final linearize at
    a lane's last pose the voxel numbers are the model's exactly."""
    w = s2m["w"]
    G = _guesses(w)[[0, 4]]
    g = _kengine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, K)
    if K == 1:
        m = _model(s2m, w.source, s2m["cs"], 1.0)
    else:
        m = _nbr_model(s2m["maps"], (1.0, None), w.source, w.target, s2m["cs"], s2m["ct"], 1.0, K)
    T, conv, its, H = g.alignBatchVoxel(G)
    full = [g.lm_trace(lane=i).copy() for i in range(2)]
    n_full = [int(i) + 1 for i in its]
    print(f"DIRECT{K}: lanes end after {n_full} iterations")
    poses, H_at = [[G[0]], [G[1]]], [{}, {}]
    for k in range(1, max(n_full) + 1):
        g.setMaximumIterations(k)
        Tk, _, _, Hk = g.alignBatchVoxel(G)
        for lane in range(2):
            if k > n_full[lane]:
                continue
            where = f"DIRECT{K} lane {lane}: pass {k} of {n_full[lane]}"
            tr = g.lm_trace(lane=lane)
            n_rows = int(np.sum(full[lane][:, 0] < k))
            assert tr.shape == (n_rows, 8) and np.array_equal(tr, full[lane][:n_rows]), f"{where}: the LM trace is not a prefix of the full run's"
            Hm, _, em = m.linearize(poses[lane][k - 1].astype(np.float64))
            rows = tr[tr[:, 0] == k - 1]
            assert len(rows), where
            for y0 in rows[:, 2]:
                assert _rel(y0, em) <= H_TOL, f"{where}: y0 {y0!r} vs the model's {em!r}"
            dE = max(_rel(y, em) for y in rows[:, 2])
            if rows[-1, 7] == 1:
                yo = m.compute_error(Tk[lane].astype(np.float64))
                dE = max(dE, _rel(rows[-1, 3], yo))
                assert _rel(rows[-1, 3], yo) <= H_TOL, f"{where}: yi {rows[-1, 3]!r} of the accepted trial vs the model's {yo!r}"
            H_at[lane][k - 1] = Hm
            if tr[-1, 7] == 0:  # ended on a rejected trial: the pose stayed, H is that of the last accepted step
                assert np.array_equal(Tk[lane], poses[lane][k - 1]), f"{where}: a rejected trial moved the pose"
                n_acc = int(tr[:, 7].sum())
                Href = H_at[lane][n_acc - 1] if n_acc else np.eye(6)
            else:
                Href = Hm
            dH = float(np.abs(Hk[lane] - Href).max() / np.abs(Href).max())
            print(f"{where}: |dH|/|H| {dH:.1e}, y0/yi rel. {dE:.1e}")
            assert dH <= H_TOL, f"{where}: |dH|/|H| = {dH:.2e}"
            poses[lane].append(Tk[lane].copy())
    for lane in range(2):
        assert np.array_equal(poses[lane][-1], T[lane])
        P = T[lane].astype(np.float64)
        g.linearize(P)
        m.linearize(P)
        cn = g.voxel_correspondences()
        want = m.corr[:, None] if K == 1 else m.corr_n
        assert cn.shape == want.shape and np.array_equal(cn, want), f"DIRECT{K} lane {lane}: voxel numbers differ"
        assert (cn >= 0).any()
    g.close()


# ---- 4. hygiene -------------------------------------------------------------------------------------------------------------------
def _snapshot(g, T=None):
    """What the getters return; with T also compute_error(T), which needs a linearize on the handle."""
    st = g.stats()
    st.pop("device_allocs")  # (a count of this PROCESS's hipMalloc calls, documented to move with any call that grows a buffer)
    out = (g.getFinalTransformation().copy(), bool(g.hasConverged()), int(g.nr_iterations_), g.getFinalHessian().copy(), g.lm_trace().copy(),
           *g.correspondences(), g.voxel_correspondences())
    if T is not None:
        out += (np.float64(g.compute_error(T)),)
    return out + (st,)


def _assert_same_snapshot(a, b):
    assert len(a) == len(b)
    for x, y in zip(a[:-1], b[:-1]):
        assert _same_bits(np.asarray(x), np.asarray(y))
    assert a[-1] == b[-1], {k: (a[-1][k], b[-1][k]) for k in a[-1] if a[-1][k] != b[-1][k]}


@pytest.mark.parametrize("K", KS)
def test_the_batch_leaves_the_results_of_the_last_align_alone(ng, s2m, K):
    w = s2m["w"]
    G = _guesses(w)
    g = _kengine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, K)
    g.align(w.guess)
    before = _snapshot(g)
    g.alignBatchVoxel(G)
    _assert_same_snapshot(before, _snapshot(g))
    # ... also when nothing of the align had been fetched before the batch, and the batch runs with larger budgets than the align did
    g.align(w.guess)
    stats = g.stats()  # (align_ms and the like are this align's)
    stats.pop("device_allocs")
    g.setMaximumIterations(300); g.setLMMaxIterations(40)
    g.alignBatchVoxel(G[:3])
    _assert_same_snapshot(before[:-1] + (stats,), _snapshot(g))
    # ... and the state compute_error evaluates, frozen by a linearize, with the correspondences of that linearize
    g.linearize(_f32_pose((0.3, 0.1, 0.02), (0.5, -0.3, 2.0)))
    T2 = _f32_pose((0.31, 0.09, 0.02), (0.5, -0.3, 2.0))
    frozen = _snapshot(g, T2)
    g.alignBatchVoxel(G)
    _assert_same_snapshot(frozen, _snapshot(g, T2))
    for x, y in zip(frozen[:5], before[:5]):  # (the linearize hook leaves the align's results where they are, too)
        assert _same_bits(np.asarray(x), np.asarray(y))
    g.close()


def test_the_map_is_built_once_per_batch_at_most(ng, s2m):
    w = s2m["w"]
    G = _guesses(w)
    g = _kengine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, 7)
    assert g.voxelMapBuilds() == 0
    g.alignBatchVoxel(G)
    assert g.voxelMapBuilds() == 1  # not once per lane
    g.alignBatchVoxel(G)
    assert g.voxelMapBuilds() == 1
    g.setNeighborSearchMethod(27)  # the map does not depend on the neighbourhood
    g.alignBatchVoxel(G)
    assert g.voxelMapBuilds() == 1
    g.setInputTarget(w.target); g.setTargetCovariances(s2m["ct"])
    g.alignBatchVoxel(G[:2])
    assert g.voxelMapBuilds() == 2
    g.alignBatchVoxel(G[:2])
    assert g.voxelMapBuilds() == 2
    g.close()


def test_errors(ng, s2m):
    w = s2m["w"]
    G = _guesses(w)
    g = _kengine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 0, 7)  # the mode is off
    with pytest.raises(ng.NgicpError) as e:
        g.alignBatchVoxel(G)
    assert e.value.code == -3  # NGICP_ERR_STATE
    T_exact = g.alignBatch(G[:2])[0]
    g.setVoxelResolution(1.0)
    with pytest.raises(ng.NgicpError) as e:  # the exact entry stays refused
        g.alignBatch(G)
    assert e.value.code == -2 and "not available with a voxelized target" in str(e.value)
    for B in (0, ng.BATCH_MAX_LANES + 1):
        with pytest.raises(ng.NgicpError) as e:
            g.alignBatchVoxel(np.repeat(G[:1], B, 0))
        assert e.value.code == -2  # NGICP_ERR_ARG
    _batch_then_singles(g, G[:3], "after the errors")  # the handle is still usable
    g.setVoxelResolution(0)
    assert np.array_equal(g.alignBatch(G[:2])[0], T_exact)
    g.close()
    g = ng.NanoGICP()
    g.setVoxelResolution(1.0)
    with pytest.raises(ng.NgicpError) as e:  # neither cloud: as align
        g.alignBatchVoxel(G)
    assert e.value.code == -3
    g.close()


def test_resolution_zero_restores_exact_gicp_bit_for_bit_after_a_voxel_batch(ng, s2m):
    w = s2m["w"]
    g = _engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 0, setMaxCorrespondenceDistance=w.max_corr_dist)
    g.align(w.guess)
    want = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), *g.correspondences())
    for K in KS:
        g.setVoxelResolution(1.0)
        g.setNeighborSearchMethod(K)
        g.alignBatchVoxel(_guesses(w))
        g.setVoxelResolution(0)
        g.align(w.guess)
        got = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), *g.correspondences())
        for x, y in zip(got, want):
            assert _same_bits(x, y), K
    g.close()


def test_voxel_batches_from_two_threads_give_the_serial_results(ng, s2m):
    w = s2m["w"]
    G = _guesses(w)
    sets = [G, G[::-1].copy()]
    ref = _kengine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, 7)
    refs = _single(ref, G)
    ref.close()
    want = [refs, refs[::-1]]
    results, errors = [None, None], []

    def work(t):
        try:
            g = _kengine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, 7)
            out = []
            for _ in range(3):
                res = g.alignBatchVoxel(sets[t])
                out.append((res, [g.lm_trace(lane=i) for i in range(len(sets[t]))]))
            g.close()
            results[t] = out
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not errors, errors
    assert all(not th.is_alive() for th in threads)
    for t in range(2):
        for res, traces in results[t]:
            _assert_lanes_equal(res, traces, want[t], f"thread {t}")


# ---- 5. the selection recipe --------------------------------------------------------------------------------------------------------
def test_lowest_fitness_picks_the_minimum_the_workload_s_guess_reaches(ng):
    """INTEGRATION.md, "More than one candidate pose", voxelized: align the twelve guesses of tests/_batch_cases.py, score the results with
    fitnessBatch, take the lowest.  tests/test_vgicp_batch_cpu.py shows on the numpy model that this separates the minima at the
    resolution and settings of tests/_vgicp_batch_cases.py; here the engine does it."""
    w = bc.workload()
    G = bc.guesses(w)
    g = ng.NanoGICP()
    vbc.configure(g)
    g.setInputSource(w.source); g.setInputTarget(w.target)
    T, conv, its, _ = g.alignBatchVoxel(G)
    scores, cnt = g.fitnessBatch(T, vbc.MAX_RANGE)
    best = int(np.argmin(scores))
    print("iterations", its.tolist(), "converged", conv.astype(int).tolist())
    print("fitness", ["%.4g" % s for s in scores], cnt.tolist(), "-> lane", best)
    print("pose error against lane 0:", ["%.2e m %.2e rad" % clouds.pose_error(t, T[0]) for t in T])
    dt, dr = clouds.pose_error(T[best], T[0])
    assert dt <= TOL_T and dr <= TOL_R, (best, dt, dr)
    wrong = [i for i, t in enumerate(T) if not (clouds.pose_error(t, T[0])[0] <= TOL_T and clouds.pose_error(t, T[0])[1] <= TOL_R)]
    assert wrong, "every lane reached the same minimum: the pick shows nothing"
    g.close()
