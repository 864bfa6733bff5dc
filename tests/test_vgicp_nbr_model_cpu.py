"""The numpy model of the DIRECT7 / DIRECT27 neighbourhoods (tests/_vgicp_nbr_model.py) proving itself without a GPU: at K = 1 it IS
the DIRECT1 model, its slots are consistent between the neighbourhoods, and its H and b are the derivatives of its own error."""
import os
import re

import numpy as np
import pytest

import _vgicp_model as vm
import _vgicp_nbr_model as nm
from direct_lidar_odometry_amd import clouds
from test_vgicp_model_cpu import _perturbed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(K, seed=0, n_tgt=1500, n_src=400, res=1.0, **kw):
    """test_vgicp_model_cpu._scene's cloud (the same draws in the same order) under neighbourhood K."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-6, 6, (n_tgt, 3)).astype(np.float32)
    A = rng.normal(0, 0.1, (n_tgt, 3, 3))
    ct = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    src = (tgt[rng.permutation(n_tgt)[:n_src]] + rng.normal(0, 0.05, (n_src, 3))).astype(np.float32)
    B = rng.normal(0, 0.1, (n_src, 3, 3))
    cs = B @ B.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return nm.VoxelGICPNbrModel(src, tgt, cs, ct, res, neighbors=K, **kw)


def test_the_offset_tables():
    assert [len(nm.OFFSETS[k]) for k in (1, 7, 27)] == [1, 7, 27]
    assert nm.OFFSETS[7][0] == (0, 0, 0) and nm.OFFSETS[27][13] == (0, 0, 0) and nm.CENTRE == {1: 0, 7: 0, 27: 13}
    # DIRECT27: ascending (dz, dy, dx), dx fastest - the order of the voxel key
    assert list(nm.OFFSETS[27]) == [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    key = [(dz * (1 << 42)) + (dy * (1 << 21)) + dx for dx, dy, dz in nm.OFFSETS[27]]
    assert key == sorted(key)
    assert set(nm.OFFSETS[7]) == {o for o in nm.OFFSETS[27] if sum(map(abs, o)) <= 1}
    assert list(nm.OFFSETS[7][1:]) == [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def test_k1_is_the_direct1_model_exactly():
    a, b = _scene(1), _scene(1)
    b.__class__ = vm.VoxelGICPModel  # the same data under the parent's methods
    T = clouds.make_pose((0.05, -0.02, 0.03), (0.5, -0.4, 0.8))
    Ha, ba, ea = a.linearize(T)
    Hb, bb, eb = b.linearize(T)
    assert a.corr_n.shape == (400, 1) and np.array_equal(a.corr_n[:, 0], b.corr) and np.array_equal(a.corr, b.corr) and np.array_equal(a.sqd, b.sqd)
    assert np.array_equal(Ha, Hb) and np.array_equal(ba, bb) and ea == eb
    T2 = _perturbed(T, [1e-3, -2e-3, 5e-4, 0.01, -0.02, 0.005])
    assert a.compute_error(T2) == b.compute_error(T2)
    guess = clouds.make_pose((0.2, -0.1, 0.05), (1, -1, 2)).astype(np.float32)
    Ta, Tb = a.align(guess), b.align(guess)
    assert np.array_equal(Ta, Tb) and len(a.trace) > 0 and np.array_equal(np.asarray(a.trace), np.asarray(b.trace))
    assert (a.converged, a.nr_iterations) == (b.converged, b.nr_iterations)


def test_the_slots_of_direct7_are_those_of_direct27_and_slot_0_is_direct1():
    g1, g7, g27 = _scene(1), _scene(7), _scene(27)
    far = np.array([[100, 100, 100], [np.nan, 0, 0], [3e7, 0, 0]], np.float32)
    for g in (g1, g7, g27):
        g.src = np.r_[g.src, far]
        g.ca = np.r_[g.ca, np.repeat(np.eye(3)[None], 3, 0)]
    T = clouds.make_pose((0.05, -0.02, 0.03), (0.5, -0.4, 0.8))
    for g in (g1, g7, g27):
        g.update_correspondences(T)
    for s, off in enumerate(nm.OFFSETS[7]):
        assert np.array_equal(g7.corr_n[:, s], g27.corr_n[:, nm.OFFSETS[27].index(off)]), off
    assert np.array_equal(g7.corr_n[:, 0], g1.corr_n[:, 0]) and np.array_equal(g27.corr, g1.corr) and np.array_equal(g7.sqd, g1.sqd)
    assert (g27.corr_n[-3:] == -1).all() and (g27.corr_n >= 0).sum() > (g7.corr_n >= 0).sum() > (g1.corr_n >= 0).sum() > 0
    # a slot's voxel is the centre's voxel moved by the slot's offset
    c = vm.voxel_of(g27.q, 1.0)
    for s, off in enumerate(nm.OFFSETS[27]):
        rows = np.flatnonzero(g27.corr_n[:, s] >= 0)
        assert (g27.vmap.ijk[g27.corr_n[rows, s]] == c[rows] + np.asarray(off)).all()


def test_the_range_edge_is_tested_on_the_integers():
    L = vm.VOXEL_LIMIT
    tgt = np.array([[L - 0.5, 0.5, 0.5], [L - 1.5, 0.5, 0.5], [-(L - 1.5), 0.5, 0.5], [-(L - 2.5), 0.5, 0.5]], np.float32)  # (floor: -(L - 1.5) is in voxel -(L - 1))
    m = vm.VoxelMap(tgt, np.repeat(np.eye(3)[None], 4, 0), 1.0)
    assert m.ijk[:, 0].tolist() == [-(L - 1), -(L - 2), L - 2, L - 1]
    q = np.array([[L - 0.5, 0.5, 0.5], [-(L - 1.5), 0.5, 0.5], [L + 0.5, 0.5, 0.5], [-(L - 0.5), 0.5, 0.5]], np.float32)
    c7 = nm.lookup_slots(m, q, 7)
    assert c7[0].tolist() == [3, -1, 2, -1, -1, -1, -1]   # +x would be voxel 2^20: out of range, not a wrap into the y field
    assert c7[1].tolist() == [0, 1, -1, -1, -1, -1, -1]   # -x would be -2^20
    assert (c7[2:] == -1).all()                           # the centre itself is out of range (2^20, -2^20): no slot at all, not even the one towards the map
    c27 = nm.lookup_slots(m, q, 27)
    assert c27[0, [12, 13, 14]].tolist() == [2, 3, -1] and c27[1, [12, 13, 14]].tolist() == [-1, 0, 1] and (c27[2:] == -1).all()


@pytest.mark.parametrize("K", [7, 27])
def test_b_is_half_the_gradient_of_err(K):
    """test_vgicp_model_cpu's method and tolerance: central differences of err under frozen voxels and frozen matrices, step 1e-4,
    tolerance h^2 (1 + r^2) fixed from the step (the derivation is in that test's docstring; a sum over slots changes nothing in it)."""
    g = _scene(K)
    T = clouds.make_pose((0.05, -0.02, 0.03), (0.5, -0.4, 0.8))
    H, b, err = g.linearize(T)
    assert np.abs(H - H.T).max() <= 1e-15 * np.abs(H).max()
    assert ((g.corr_n >= 0).sum(axis=1) > 1).sum() > 100
    h = 1e-4
    r = float(np.abs(g.src).max() * np.sqrt(3) + 1.0)
    tol = h * h * (1.0 + r * r)
    grad = np.empty(6)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        grad[k] = (g.compute_error(_perturbed(T, d)) - g.compute_error(_perturbed(T, -d))) / (2 * h)
    print("b vs FD:", np.abs(grad / 2 - b).max() / np.abs(b).max(), "tolerance", tol)
    assert np.abs(grad / 2 - b).max() <= tol * np.abs(b).max()
    assert abs(g.compute_error(T) - err) <= 1e-12 * err


@pytest.mark.parametrize("K", [7, 27])
def test_H_is_half_the_hessian_of_err_where_the_residuals_vanish(K):
    """As test_vgicp_model_cpu (method, step and tolerance): H is half the Hessian of err where every residual is zero.  A point cannot
    sit on the means of several voxels at once, so the zero-residual set-up gives every point ONE pair, its own voxel's mean, and files
    it - by hand, under frozen correspondences - in a slot that changes from point to point: every slot's terms go through the model's
    sum over slots, which is what is under test."""
    g = _scene(K)
    m = g.vmap
    src = m.mean.copy()
    n = len(m)
    cs = np.repeat((0.01 * np.eye(3))[None], n, 0)
    I = np.eye(4)
    slot_of = np.arange(n) % K
    corr_n = np.full((n, K), -1, dtype=np.int64)
    corr_n[np.arange(n), slot_of] = np.arange(n)
    g.src, g.ca, g.corr_n = src, cs, corr_n  # frozen correspondences, set by hand
    H, b, err = g.accumulate(I)
    assert err == 0.0 and not b.any()
    f = lambda d: g.compute_error(_perturbed(I, d))
    h = 1e-3
    r = float(np.abs(src).max() * np.sqrt(3) + 1.0)
    tol = h * h * (1.0 + r * r)
    Hfd = np.empty((6, 6))
    for k in range(6):
        for l in range(k, 6):
            dk, dl = np.zeros(6), np.zeros(6)
            dk[k], dl[l] = h, h
            Hfd[k, l] = Hfd[l, k] = (f(dk + dl) - f(dk - dl) - f(-dk + dl) + f(-dk - dl)) / (4 * h * h) / 2
    print("H vs FD:", np.abs(Hfd - H).max() / np.abs(H).max(), "tolerance", tol)
    assert np.abs(Hfd - H).max() <= tol * np.abs(H).max()
    # and it is the sum of DIRECT1's terms over the same pairs
    H1 = vm.terms(src, cs, m, np.arange(n), I)[0]
    assert np.abs(H - H1).max() <= 1e-12 * np.abs(H1).max()


def test_the_slab_separates_the_modes():
    src, tgt, cs, ct = nm.slab()
    I = np.eye(4)
    g = {K: nm.VoxelGICPNbrModel(src, tgt, cs, ct, 1.0, neighbors=K) for K in (1, 7, 27)}
    for m in g.values():
        m.update_correspondences(I)
    assert (g[1].corr_n == -1).all()
    assert (g[7].corr_n >= 0).sum(axis=0).tolist() == [0, 0, 257, 0, 0, 0, 0]
    n27 = (g[27].corr_n >= 0).sum(axis=0)
    assert n27[13] == 0 and n27[12] == 257
    assert all((n27[s] > 0) <= (nm.OFFSETS[27][s][0] == -1) for s in range(27)) and n27.sum() > 257
    # slot 2 of DIRECT7 is the voxel the very same point lies in, as a target point
    own = g[7].vmap.lookup(tgt[:257])
    assert np.array_equal(g[7].corr_n[:, 2], own)
    # DIRECT1 sees nothing: H = 0; DIRECT7 sees the wall
    assert not g[1].accumulate(I)[0].any() and g[7].accumulate(I)[2] > 0


def test_header_binding_and_shim_declare_the_entries():
    hdr = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    from direct_lidar_odometry_amd import nano_gicp
    for name in ("ngicp_set_voxel_neighbors", "ngicp_get_voxel_neighbors", "ngicp_voxel_correspondences", "ngicp_voxelmap_builds"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in nano_gicp.EXPORTS
    for name, val in (("NGICP_VOX_DIRECT1", 1), ("NGICP_VOX_DIRECT7", 7), ("NGICP_VOX_DIRECT27", 27)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    assert [int(v) for v in nano_gicp.NeighborSearchMethod] == [1, 7, 27]
    for m in ("setNeighborSearchMethod", "getNeighborSearchMethod", "voxel_correspondences"):
        assert hasattr(nano_gicp.NanoGICP, m)
    shim = open(os.path.join(ROOT, "include", "nano_gicp", "nano_gicp.hpp")).read()
    assert re.search(r"enum class NeighborSearchMethod\s*\{\s*DIRECT1 = 1, DIRECT7 = 7, DIRECT27 = 27\s*\}", shim)
    for m in ("setNeighborSearchMethod", "getNeighborSearchMethod", "voxelCorrespondences"):
        assert m in shim
