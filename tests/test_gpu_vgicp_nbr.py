"""The DIRECT7 / DIRECT27 neighbourhoods of voxelized GICP on the GPU (ngicp_set_voxel_neighbors; k_vgicp_pass_n in csrc/ngicp_voxel.h)
against the numpy model of their definition (tests/_vgicp_nbr_model.py, which proves itself in test_vgicp_nbr_model_cpu.py).
Tolerances are the project's for the same quantities (test_gpu_vgicp.py): voxel numbers exact, H / b / err / compute_error within 1e-9 of
the largest entry, per-pass y0 / yi / H within _pass_check.H_TOL."""
import numpy as np
import pytest

import _vgicp_model as vm
import _vgicp_nbr_model as nm
from _pass_check import H_TOL
from direct_lidar_odometry_amd import clouds
from test_gpu_vgicp import ALIGN_CASES, _close, _engine, _f32_pose, _half_the_voxels_negative, _rel, _spd, ng, s2m  # noqa: F401  (ng, s2m: fixtures)

pytestmark = pytest.mark.gpu

KS = (7, 27)
# Which half of the voxels gets the covariance -2 I in the LM-rejection cases.  Summing a point's terms over its neighbours mixes voxels
# of either sign and smooths the cost, so a RANDOM half rejects far more rarely than under DIRECT1.  On the CPU model (with
# _vgicp_model.plane_covariances for the engine's): under DIRECT7 the draws 9 and 14 of the seeds 0..15 reject (8 of 14 trials; 4 of 5 with
# four trials per iteration), under DIRECT27 none of the seeds 0..63 rejects a single trial - a point's 27 voxels are never mostly of
# one sign.  DIRECT27 therefore gets a CONTIGUOUS half, the voxels whose iy lies below the median iy of the occupied ones: there the
# neighbourhoods are of one sign except along one plane, and the model accepts the first trial, rejects nine in the next iteration
# and accepts the tenth (with four trials per iteration it ends on four rejected ones).
HALF_NEGATIVE_SEED = 9


def _half_negative(s2m, res, K):
    """-> (target covariances with half of the voxels at -2 I, the tag of that half for the cache of model maps)."""
    if K != 27:
        return _half_the_voxels_negative(s2m, res, seed=HALF_NEGATIVE_SEED), ("half_negative", HALF_NEGATIVE_SEED)
    ijk = vm.voxel_of(s2m["w"].target, res)
    below = ijk[:, 1] < np.median(np.unique(ijk, axis=0)[:, 1])
    ct = s2m["ct"].copy()
    ct[below, :3, :3] = -2.0 * np.eye(3)
    share = float(len(np.unique(ijk[below], axis=0))) / len(np.unique(ijk, axis=0))
    assert 0.4 < share < 0.6, share  # about half of the voxels
    return ct, ("half_negative", "iy below the median")


def _nbr_engine(ng, src, tgt, cs, ct, res, K, **settings):
    g = _engine(ng, src, tgt, cs, ct, res, **settings)
    g.setNeighborSearchMethod(K)
    return g


def _nbr_model(cache, key, src, tgt, cs, ct, res, K):
    """The model on `tgt`; voxel maps are built once per `key` in `cache` and shared."""
    m = nm.VoxelGICPNbrModel.__new__(nm.VoxelGICPNbrModel)
    vm.NumpyGICP.__init__(m, src, tgt, cs, ct)
    if key not in cache:
        cache[key] = vm.VoxelMap(m.tgt, ct, res)
    m.vmap = cache[key]
    m.set_neighbors(K)
    return m


def _check_linearisation(g, m, T, label):
    H, b, err = g.linearize(T)
    Hm, bm, em = m.linearize(T)
    cn = g.voxel_correspondences()
    assert cn.shape == m.corr_n.shape and cn.dtype == np.int32
    assert np.array_equal(cn, m.corr_n), f"{label}: voxel numbers differ at {np.argwhere(cn != m.corr_n)[:5].tolist()}"
    corr, sqd = g.correspondences()  # the centre slot's
    assert np.array_equal(corr, m.corr) and np.array_equal(sqd, m.sqd), label
    if (m.corr_n >= 0).any():
        _close(H, Hm, 1e-9, f"{label}: H"); _close(b, bm, 1e-9, f"{label}: b"); _close([err], [em], 1e-9, f"{label}: err")
    else:
        assert not H.any() and not b.any() and err == 0.0, label
    assert np.array_equal(H, H.T)
    return H, b, err


def _check_every_pass(g, fresh, m, guess, max_iter, gn, case):
    """test_gpu_vgicp.test_every_pass_of_an_alignment_matches_the_model's method under a neighbourhood: align(max_iter = k) for every k up
    to the full run; at the pose of every trace row's linearisation the (n, K) voxel numbers are exact and y0 / yi / H are within H_TOL.
    Then the run is repeated on this handle and on `fresh`: bit-identical.  -> (final pose, trace, iterations)."""
    guess = np.asarray(guess, np.float32)
    g.setMaximumIterations(max_iter)
    g.align(guess)
    full = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), g.nr_iterations_, g.converged_)
    n_full = g.nr_iterations_ + 1
    print(f"{case}: {n_full} iterations, converged {g.converged_}, {int((full[1][:, 7] == 0).sum()) if len(full[1]) else 0} rejected trials")
    poses, H_at = [guess], {}
    Hg = full[2]
    for k in range(1, n_full + 1):
        where = f"{case}: pass {k} of {n_full}"
        g.setMaximumIterations(k)
        g.align(guess)
        T, Hg, tr = g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.lm_trace().copy()
        cn = g.voxel_correspondences()
        corr, sqd = g.correspondences()
        P = poses[k - 1].astype(np.float64)
        Hm, _, em = m.linearize(P)
        assert np.array_equal(cn, m.corr_n), f"{where}: voxel numbers differ at {np.argwhere(cn != m.corr_n)[:5].tolist()}"
        assert np.array_equal(corr, m.corr) and np.array_equal(sqd, m.sqd), where
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
        print(f"{where}: pairs per point {(cn >= 0).mean() * cn.shape[1]:.3f}, |dH|/|H| {dH:.1e}, y0/yi rel. {dE:.1e}")
        assert dH <= H_TOL, f"{where}: |dH|/|H| = {dH:.2e}"
        n_rows = int(np.sum(full[1][:, 0] < k)) if len(full[1]) else 0
        assert tr.shape == (n_rows, 8) and np.array_equal(tr, full[1][:n_rows]), f"{where}: the LM trace is not a prefix of the full run's"
        poses.append(T)
    assert np.array_equal(poses[-1], full[0]) and np.array_equal(Hg, full[2]) and (g.nr_iterations_, g.converged_) == full[3:]
    for e in (g, fresh):
        e.setMaximumIterations(max_iter)
        e.align(guess)
        assert np.array_equal(e.getFinalTransformation(), full[0]) and np.array_equal(e.lm_trace(), full[1]) and np.array_equal(e.getFinalHessian(), full[2])
        assert (e.nr_iterations_, e.converged_) == full[3:]
    return full[0], full[1], n_full


# ---- 1. the slab: the case that separates the modes -------------------------------------------------------------------------------
def test_the_slab_separates_the_modes(ng):
    src, tgt, cs, ct = nm.slab()
    I = np.eye(4)
    cache = {}
    counts = {}
    for K in (1, 7, 27):
        g = _nbr_engine(ng, src, tgt, cs, ct, 1.0, K)
        m = _nbr_model(cache, "slab", src, tgt, cs, ct, 1.0, K)
        _check_linearisation(g, m, I, f"slab DIRECT{K}")
        counts[K] = (g.voxel_correspondences() >= 0).sum(axis=0)
        assert np.array_equal(counts[K], (m.corr_n >= 0).sum(axis=0))
        if K == 1:  # blind: nothing to align against, the pose stays where it was
            g.align(I.astype(np.float32))
            assert np.array_equal(g.getFinalTransformation(), np.eye(4, dtype=np.float32))
        g.close()
    print("slab pairs per slot:", {K: c.tolist() for K, c in counts.items()})
    # what the model's counts are (test_vgicp_nbr_model_cpu.test_the_slab_separates_the_modes pins them on the CPU)
    assert counts[1].sum() == 0 and counts[7][2] == 257 == counts[7].sum() and counts[27][13] == 0 and counts[27][12] == 257
    assert all(counts[27][s] == 0 for s in range(27) if nm.OFFSETS[27][s][0] != -1)
    # from that pose DIRECT7 aligns, pass for pass as the model
    g = _nbr_engine(ng, src, tgt, cs, ct, 1.0, 7)
    f = _nbr_engine(ng, src, tgt, cs, ct, 1.0, 7)
    m = _nbr_model(cache, "slab", src, tgt, cs, ct, 1.0, 7)
    T, tr, n_it = _check_every_pass(g, f, m, I, 64, False, "slab DIRECT7")
    assert not np.array_equal(T, np.eye(4, dtype=np.float32)) and T[0, 3] < -0.5  # towards the wall, one voxel back
    g.close(); f.close()


# ---- 2. linearize / compute_error against the model -------------------------------------------------------------------------------
def _negative_target(s2m):
    """The shared target moved so that every coordinate of it, and of a source aligned to it, is negative: floorf, not truncation, decides
    the voxels and their neighbours."""
    if "neg" not in s2m:
        w = s2m["w"]
        shift = -np.ceil(np.abs(np.r_[w.target, w.source]).max() + 8.0)
        s2m["neg"] = (np.ascontiguousarray(w.target + np.float32(shift)), float(shift))
    return s2m["neg"]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("res", [0.5, 2.0])
@pytest.mark.parametrize("n_src", [1, 255, 256, 257, 513])
def test_linearize_and_compute_error_match_the_model(ng, s2m, n_src, res, K):
    w = s2m["w"]
    extra = np.array([[500, 500, 500], [3e6, 0, 0], [0.3, 0.2, 40.0]], np.float32)  # far away; beyond 2^20 voxels at either resolution; above the room
    if n_src == 1:
        src, cs = np.ascontiguousarray(w.source[1500:1501]), s2m["cs"][1500:1501]
    else:
        pick = np.linspace(0, 3007, n_src - 3).astype(int)
        src, cs = np.ascontiguousarray(np.r_[w.source[pick], extra]), np.r_[s2m["cs"][pick], _spd(3, 60)]
    assert len(src) == n_src
    maps = s2m["maps"]
    g = _nbr_engine(ng, src, w.target, cs, s2m["ct"], res, K)
    m = _nbr_model(maps, (res, None), src, w.target, cs, s2m["ct"], res, K)
    for T in (_f32_pose((0.3, 0.1, 0.02), (0.5, -0.3, 2.0)), np.eye(4)):
        _check_linearisation(g, m, T, f"n {n_src} res {res} DIRECT{K}")
        if n_src > 1:
            assert (m.corr_n[-3:] == -1).all() and ((m.corr_n >= 0).sum(axis=1) > 1).any()
        T2 = (_f32_pose((0.01, -0.02, 0.005), (0.1, 0.05, -0.2)) @ T).astype(np.float32).astype(np.float64)  # a second pose for compute_error
        _close([g.compute_error(T2)], [m.compute_error(T2)], 1e-9, "compute_error")
    g.close()
    # negative coordinates throughout
    tneg, shift = _negative_target(s2m)
    Tn = _f32_pose((0.3 + shift, 0.1 + shift, 0.02 + shift), (0.5, -0.3, 2.0))
    g = _nbr_engine(ng, src, tneg, cs, s2m["ct"], res, K)
    m = _nbr_model(maps, (res, "neg"), src, tneg, cs, s2m["ct"], res, K)
    _check_linearisation(g, m, Tn, f"n {n_src} res {res} DIRECT{K} negative")
    inside = m.q[: 1 if n_src == 1 else -3]
    assert (inside < 0).all() and (m.vmap.ijk < 0).all() and (n_src == 1 or (m.corr_n >= 0).any())
    T2 = (_f32_pose((0.01, -0.02, 0.005), (0.1, 0.05, -0.2)) @ Tn).astype(np.float32).astype(np.float64)
    _close([g.compute_error(T2)], [m.compute_error(T2)], 1e-9, "compute_error, negative")
    g.close()


# ---- 3. occupancy extremes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_a_full_lattice_fills_every_slot(ng, K):
    c = np.arange(5, dtype=np.float32) + np.float32(0.5)
    tgt = np.ascontiguousarray(np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3))  # one point per voxel of a 5 x 5 x 5 block
    ct = _spd(125, 80)
    src = np.array([[2.4, 2.6, 2.5], [0.4, 0.6, 0.5], [4.6, 4.4, 4.5], [0.5, 4.5, 0.5], [1.5, 2.5, 3.5], [0.5, 2.5, 2.5]], np.float32)
    cs = _spd(len(src), 81)
    g = _nbr_engine(ng, src, tgt, cs, ct, 1.0, K)
    m = _nbr_model({}, "lattice", src, tgt, cs, ct, 1.0, K)
    assert len(m.vmap) == 125 and (m.vmap.count == 1).all()
    _check_linearisation(g, m, np.eye(4), f"lattice DIRECT{K}")
    occupied = (g.voxel_correspondences() >= 0).sum(axis=1).tolist()
    assert occupied == ([27, 8, 8, 8, 27, 18] if K == 27 else [7, 4, 4, 4, 7, 6]), occupied
    T2 = _f32_pose((0.05, -0.04, 0.03), (1, -2, 3))
    _close([g.compute_error(T2)], [m.compute_error(T2)], 1e-9, "compute_error")
    g.close()


@pytest.mark.parametrize("K", KS)
def test_a_single_voxel_target(ng, K):
    tgt = np.random.default_rng(82).uniform(0.05, 0.95, (300, 3)).astype(np.float32)
    ct = _spd(300, 83)
    # inside the voxel, in its face / edge / corner neighbours, and two voxels away
    src = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, -0.5], [1.5, 1.5, 0.5], [-0.5, -0.5, -0.5], [2.5, 0.5, 0.5], [0.5, -1.5, 0.5]],
                   np.float32)
    cs = _spd(len(src), 84)
    g = _nbr_engine(ng, src, tgt, cs, ct, 1.0, K)
    m = _nbr_model({}, "one", src, tgt, cs, ct, 1.0, K)
    assert len(m.vmap) == 1
    _check_linearisation(g, m, np.eye(4), f"one voxel DIRECT{K}")
    occupied = (g.voxel_correspondences() >= 0).sum(axis=1).tolist()
    assert occupied == ([1, 1, 1, 1, 1, 1, 1, 0, 0] if K == 27 else [1, 1, 1, 1, 1, 0, 0, 0, 0]), occupied
    g.close()


@pytest.mark.parametrize("K", KS)
def test_a_source_outside_the_map_behaves_as_exact_gicp_without_correspondences(ng, s2m, K):
    """test_gpu_vgicp's test of this name, under a neighbourhood: align() when no slot of any point has a voxel."""
    w = s2m["w"]
    src = np.ascontiguousarray(w.source[:500])

    def outcome(g):
        g.align()
        return (g.getFinalTransformation().copy(), g.converged_, g.nr_iterations_, g.getFinalHessian().copy(), g.lm_trace().copy())

    ex = ng.NanoGICP()
    ex.setMaxCorrespondenceDistance(1e-6)
    ex.setInputSource(src); ex.setInputTarget(w.target[:500] + np.float32(80))
    want = outcome(ex)
    g = _nbr_engine(ng, src + np.float32(300), w.target, s2m["cs"][:500], s2m["ct"], 1.0, K)
    H, b, err = g.linearize(np.eye(4))
    assert not H.any() and not b.any() and err == 0.0 and (g.correspondences()[0] == -1).all() and (g.voxel_correspondences() == -1).all()
    assert g.voxel_correspondences().shape == (500, K)
    got = outcome(g)
    for a, e in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(e), equal_nan=True)
    ex.close(); g.close()


# ---- 4. the range edge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("sign", [1, -1])
def test_the_range_edge(ng, K, sign):
    """Voxels ix = +-(2^20 - 1) and +-(2^20 - 2) at 1 m: the slot that would be voxel +-2^20 is -1 (not a carry into the key's y field), the
    others are the model's; a source point whose own voxel is out of range has no slot at all."""
    L = float(vm.VOXEL_LIMIT)
    rng = np.random.default_rng(90)
    lo = (L - 1.0) if sign > 0 else -L + 1.0  # the lower edge of the outermost voxel in range
    inner = lo - sign * 1.0
    yz = rng.uniform(0.1, 0.9, (24, 2))
    x = np.r_[lo + rng.uniform(0.1, 0.9, 12), inner + rng.uniform(0.1, 0.9, 12)]
    tgt = np.ascontiguousarray(np.c_[x, yz].astype(np.float32))
    ct = _spd(24, 91)
    beyond = (L + 0.5) if sign > 0 else -L - 0.5
    src = np.array([[lo + 0.5, 0.5, 0.5], [beyond, 0.5, 0.5], [inner + 0.5, 0.5, 0.5], [lo + 0.25, 1.5, 0.5]], np.float32)
    cs = _spd(4, 92)
    g = _nbr_engine(ng, src, tgt, cs, ct, 1.0, K)
    m = _nbr_model({}, "edge", src, tgt, cs, ct, 1.0, K)
    edge = sign * (vm.VOXEL_LIMIT - 1)
    assert sorted(m.vmap.ijk[:, 0].tolist()) == sorted([edge, edge - sign]) and len(m.vmap) == 2
    _check_linearisation(g, m, np.eye(4), f"edge {sign:+d} DIRECT{K}")
    cn = g.voxel_correspondences()
    v_edge, v_inner = m.vmap._index[(edge, 0, 0)], m.vmap._index[(edge - sign, 0, 0)]
    out_slot = nm.OFFSETS[K].index((sign, 0, 0))
    in_slot = nm.OFFSETS[K].index((-sign, 0, 0))
    assert cn[0, nm.CENTRE[K]] == v_edge and cn[0, in_slot] == v_inner and cn[0, out_slot] == -1 and (cn[0] >= 0).sum() == 2
    assert (cn[1] == -1).all()
    assert cn[2, nm.CENTRE[K]] == v_inner and cn[2, out_slot] == v_edge and (cn[2] >= 0).sum() == 2
    assert cn[3, nm.OFFSETS[K].index((0, -1, 0))] == v_edge and cn[3, out_slot] == -1
    g.close()


# ---- 5. every pass of whole alignments --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", sorted(ALIGN_CASES))
def test_every_pass_of_an_alignment_matches_the_model(ng, s2m, case, K):
    """The case table of test_gpu_vgicp.test_every_pass_of_an_alignment_matches_the_model (its docstring explains the method and what the
    rejection cases pin), under DIRECT7 and DIRECT27.  The lm_rejection cases must reject trials (asserted)."""
    settings, guess, res, ct_tag = ALIGN_CASES[case]
    settings = dict(settings)
    w = s2m["w"]
    ct, ct_tag = _half_negative(s2m, res, K) if ct_tag else (s2m["ct"], None)  # (test_gpu_vgicp caches the map of its own draw under the bare tag)
    guess = np.asarray(w.guess if guess is None else guess, np.float32)
    max_iter = settings.pop("setMaximumIterations", 64)
    gn = settings.get("setOptimizer", 1) == 0
    g = _nbr_engine(ng, w.source, w.target, s2m["cs"], ct, res, K, **settings)
    f = _nbr_engine(ng, w.source, w.target, s2m["cs"], ct, res, K, **settings)
    m = _nbr_model(s2m["maps"], (res, ct_tag), w.source, w.target, s2m["cs"], ct, res, K)
    T, tr, n_it = _check_every_pass(g, f, m, guess, max_iter, gn, f"{case} DIRECT{K}")
    if case.startswith("lm_rejection"):
        acc, it = tr[:, 7], tr[:, 0]
        assert (acc == 0).any(), f"{case}: no trial was rejected"
        if case == "lm_rejection":
            assert (acc == 1).any() and ((acc == 0) & (it > 0)).any(), f"{case}: accepted {acc.astype(int).tolist()} in iterations {it.astype(int).tolist()}"
        else:
            assert acc[-1] == 0 and not g.converged_, f"{case}: accepted {acc.astype(int).tolist()}"
    if case == "lm_defaults":
        start, end = clouds.pose_error(guess, w.gt), clouds.pose_error(T, w.gt)
        assert end[0] < start[0] and end[1] < start[1]
    g.close(); f.close()


# ---- 6. hygiene -------------------------------------------------------------------------------------------------------------------
def test_direct1_selected_explicitly_is_the_default_bit_for_bit(ng, s2m):
    w = s2m["w"]
    a = _engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0)
    b = _nbr_engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, ng.NeighborSearchMethod.DIRECT1)
    assert a.getNeighborSearchMethod() == ng.NeighborSearchMethod.DIRECT1 == b.getNeighborSearchMethod()
    out = []
    for e in (a, b):
        e.align(w.guess)
        out.append((e.getFinalTransformation().copy(), e.lm_trace().copy(), e.getFinalHessian().copy(), *e.correspondences(), e.voxel_correspondences()))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert out[0][5].shape == (len(w.source), 1) and np.array_equal(out[0][5][:, 0], out[0][3])
    a.close(); b.close()


def test_changing_the_neighbourhood_keeps_the_map_and_drops_the_correspondences(ng, s2m):
    w = s2m["w"]
    g = _engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0)
    assert g.voxelMapBuilds() == 0
    g.linearize(np.eye(4))
    assert g.voxelMapBuilds() == 1
    ms = g.stats()["voxelmap_ms"]
    before = [x.copy() for x in g.voxelMap()]
    for K in (7, 27, 7, 1):
        g.setNeighborSearchMethod(K)
        assert int(g.getNeighborSearchMethod()) == K
        for call in (g.correspondences, g.voxel_correspondences, lambda: g.compute_error(np.eye(4))):
            with pytest.raises(ng.NgicpError) as e:
                call()
            assert e.value.code == -3  # NGICP_ERR_STATE
        g.linearize(np.eye(4))
        assert g.voxel_correspondences().shape == (len(w.source), K)
        g.correspondences(); g.compute_error(np.eye(4))
        g.setNeighborSearchMethod(K)  # the value already set: nothing happens
        g.correspondences()
        g.align(w.guess)
        assert g.voxelMapBuilds() == 1 and g.stats()["voxelmap_ms"] == ms  # only a build adds to the counter
    for x, y in zip(before, g.voxelMap()):
        assert np.array_equal(x, y)
    g.setVoxelResolution(2.0)  # what does rebuild it
    g.linearize(np.eye(4))
    assert g.voxelMapBuilds() == 2
    g.close()


def test_invalid_neighbourhoods_are_refused_and_the_setting_is_remembered_while_the_mode_is_off(ng, s2m):
    w = s2m["w"]
    g = ng.NanoGICP()
    for bad in (0, -1, 2, 6, 8, 26, 28, 9):
        with pytest.raises(ng.NgicpError) as e:
            g.setNeighborSearchMethod(bad)
        assert e.value.code == -2  # NGICP_ERR_ARG
    assert int(g.getNeighborSearchMethod()) == 1
    g.setNeighborSearchMethod(ng.NeighborSearchMethod.DIRECT7)  # the mode is off: remembered
    g.setInputSource(w.source); g.setInputTarget(w.target)
    g.setSourceCovariances(s2m["cs"]); g.setTargetCovariances(s2m["ct"])
    g.linearize(np.eye(4))
    with pytest.raises(ng.NgicpError) as e:  # exact GICP: no voxel correspondences
        g.voxel_correspondences()
    assert e.value.code == -3
    g.setVoxelResolution(1.0)
    assert int(g.getNeighborSearchMethod()) == 7
    g.linearize(np.eye(4))
    assert g.voxel_correspondences().shape == (len(w.source), 7)
    g.close()


@pytest.mark.parametrize("K", KS)
def test_batch_and_sharded_entries_are_still_refused(ng, s2m, K):
    w = s2m["w"]
    g = _nbr_engine(ng, w.source, w.target, s2m["cs"], s2m["ct"], 1.0, K)
    calls = [lambda: g.alignBatch(np.repeat(np.eye(4, dtype=np.float32)[None], 2, 0)), lambda: g.sharded_begin(), lambda: g.sharded_pass(0),
             lambda: g.sharded_step(0), lambda: g.sharded_finish(), lambda: g.covsShardBegin(1), lambda: g.covsShardCompute(1, 0, 1), lambda: g.covsShardCommit(1)]
    for call in calls:
        with pytest.raises(ng.NgicpError) as e:
            call()
        assert e.value.code == -2 and "not available with a voxelized target" in str(e.value)
    g.close()


@pytest.mark.parametrize("K", KS)
def test_resolution_zero_restores_exact_gicp_bit_for_bit_with_a_neighbourhood_set(ng, s2m, K):
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
    g.setNeighborSearchMethod(K)
    g.align(w.guess)
    T_vox = g.getFinalTransformation().copy()
    assert g.voxel_correspondences().max() < g.getVoxelMapSize()
    g.setVoxelResolution(0)
    with pytest.raises(ng.NgicpError):
        g.correspondences()
    g.align(w.guess)
    assert np.array_equal(g.getFinalTransformation(), want[0]) and np.array_equal(g.lm_trace(), want[1]) and np.array_equal(g.getFinalHessian(), want[2])
    c = g.correspondences()
    assert np.array_equal(c[0], want[3][0]) and np.array_equal(c[1], want[3][1])
    assert not np.array_equal(T_vox, want[0]) and int(g.getNeighborSearchMethod()) == K
    ref.close(); g.close()
