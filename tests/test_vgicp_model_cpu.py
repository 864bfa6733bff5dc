"""The numpy model of voxelized GICP (tests/_vgicp_model.py) proving itself without a GPU and without a reference: the definition is
the project's own (include/ngicp.h, "voxelized GICP"), so the model is held to what any correct statement of it must satisfy."""
import os
import re

import numpy as np
import pytest

import _vgicp_model as vm
from direct_lidar_odometry_amd import clouds
from oracle.numpy_model import so3_exp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(seed=0, n_tgt=1500, n_src=400, res=1.0):
    """A small cloud in a 12 m cube, anisotropic covariances, a source that is the target's subset moved a little."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-6, 6, (n_tgt, 3)).astype(np.float32)
    A = rng.normal(0, 0.1, (n_tgt, 3, 3))
    ct = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    src = (tgt[rng.permutation(n_tgt)[:n_src]] + rng.normal(0, 0.05, (n_src, 3))).astype(np.float32)
    B = rng.normal(0, 0.1, (n_src, 3, 3))
    cs = B @ B.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return vm.VoxelGICPModel(src, tgt, cs, ct, res)


def _perturbed(T, d):
    """The solver's step: delta = (so3_exp(d[:3]), d[3:]) multiplied from the LEFT."""
    D = np.eye(4)
    D[:3, :3] = so3_exp(np.asarray(d[:3], float))
    D[:3, 3] = d[3:]
    return D @ T


# ---- the voxel of a point -------------------------------------------------------------------------------------------------------
def test_voxel_of_pinned_points():
    f = np.float32
    # on a lattice plane: the plane belongs to the voxel above it
    assert vm.voxel_of([[1.0, 0.25, -0.5]], 0.25).tolist() == [[4, 1, -2]]
    assert vm.voxel_of([[2.0, 4.0, -4.0]], 4.0).tolist() == [[0, 1, -1]]
    # negative coordinates round DOWN (a cast would truncate -0.1 / 1.0 to 0)
    assert vm.voxel_of([[-0.1, -1.0, -1.0001]], 1.0).tolist() == [[-1, -1, -2]]
    # -0.0f is voxel 0, like +0.0f
    assert vm.voxel_of(np.array([[-0.0, 0.0, -0.0]], f), 0.25).tolist() == [[0, 0, 0]]
    # the float just below a plane stays below it; the product is rounded to float32 BEFORE the floor
    below = np.nextafter(f(1.0), f(0.0))
    assert vm.voxel_of([[below, below, below]], 1.0).tolist() == [[0, 0, 0]]
    assert vm.voxel_of([[below, 0, 0]], 0.25).tolist() == [[3, 0, 0]]
    # 0.3 / 0.1: inv_res = 1.0f / 0.1f = 10.0f exactly, 0.3f * 10.0f = 3.0000001192... -> rounds to 3.0f -> voxel 3 (in double it is 3.0000001: also 3);
    # 0.7f * 10.0f = 6.99999988 -> rounds to 7.0f in float32: voxel 7, where double arithmetic would say 6
    assert vm.voxel_of([[0.3, 0.7, 0.0]], 0.1).tolist() == [[3, int(np.floor(f(0.7) * (f(1.0) / f(0.1)))), 0]]
    assert np.floor(f(0.7) * (f(1.0) / f(0.1))) == 7.0 and np.floor(float(f(0.7)) * 10.0) == 6.0


def test_the_2_pow_20_limit():
    ok = np.array([[1048575.5, -1048575.0, 0]], np.float32)  # ijk = (2^20 - 1, -(2^20 - 1), 0): the last voxels inside
    assert vm.voxel_of(ok, 1.0).tolist() == [[(1 << 20) - 1, -(1 << 20) + 1, 0]]
    assert len(vm.VoxelMap(ok, np.eye(3)[None], 1.0)) == 1
    for bad in ([[1048576.0, 0, 0]], [[0, -1048575.5, 0]], [[0, 0, 262144.0]]):
        res = 0.25 if bad[0][2] else 1.0
        with pytest.raises(ValueError):
            vm.VoxelMap(np.array(bad, np.float32), np.eye(3)[None], res)


def test_voxel_map_sums_and_numbering():
    m = _scene().vmap
    # ascending (iz, iy, ix)
    key = (m.ijk[:, 2] * (1 << 42)) + (m.ijk[:, 1] * (1 << 21)) + m.ijk[:, 0]
    assert (np.diff(key) > 0).all()
    assert m.count.sum() == 1500 and all((np.diff(idx) > 0).all() for idx in m.members)
    tgt = _scene().tgt.astype(np.float64)
    for v in (0, len(m) // 2, len(m) - 1):
        np.testing.assert_allclose(m.mean[v], tgt[m.members[v]].mean(0), rtol=1e-13)
        assert (vm.voxel_of(tgt[m.members[v]].astype(np.float32), 1.0) == m.ijk[v]).all()


# ---- the terms ------------------------------------------------------------------------------------------------------------------
def test_H_is_symmetric_and_b_is_half_the_gradient_of_err():
    """Under frozen correspondences and frozen matrices n_v M, err(d) = sum e(d)^T (n_v M) e(d) at the pose delta(d) * T has the
    gradient 2 b at d = 0 exactly (J is the derivative of e for the left-multiplied so3_exp step).  Central differences with step h
    have a truncation error of h^2 / 6 * err''' ; with points within r of the origin every further derivative in a rotation direction
    costs at most a factor r, so |err'''| <= r^2 |err'| and the relative error is below h^2 (1 + r^2).  Rounding adds eps * err / h,
    orders of magnitude less at h = 1e-4.  The tolerance is that bound, fixed before looking at any result."""
    g = _scene()
    T = clouds.make_pose((0.05, -0.02, 0.03), (0.5, -0.4, 0.8))
    H, b, err = g.linearize(T)
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-15 * np.abs(H).max()
    assert (g.corr >= 0).sum() > 100 and (g.corr < 0).sum() > 0
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
    assert abs(g.compute_error(T) - err) <= 1e-12 * err  # the same pose, the same matrices


def test_H_is_half_the_hessian_of_err_where_the_residuals_vanish():
    """H = sum n_v J^T M J is the Gauss-Newton matrix: half the Hessian of err up to the term e^T M d2e, which vanishes where e = 0.
    So the check is made where every residual is exactly zero: a (float64) source made of the voxel means themselves, at identity,
    under frozen correspondences.  There err(d) = d^T H d + O(|d|^3 r); the symmetric second-difference stencils cancel the odd orders,
    what is left is h^2 / 12 * err'''' <= h^2 r^2 |err''| relative.  Tolerance h^2 (1 + r^2), fixed from the step."""
    g = _scene()
    m = g.vmap
    src = m.mean.copy()
    corr = np.arange(len(m))
    cs = np.repeat((0.01 * np.eye(3))[None], len(m), 0)
    I = np.eye(4)
    H, b, err, W = vm.terms(src, cs, m, corr, I)
    assert err == 0.0 and not b.any()
    f = lambda d: vm.terms(src, cs, m, corr, I, weight=W, T_eval=_perturbed(I, d))[2]
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


def test_a_cloud_on_its_own_voxel_map_has_no_gradient_at_identity():
    """Source = target, identical covariances, identity: b = sum_v sum_{i in v} n_v J_i^T M_i (mean_v - p_i).  With ONE covariance for
    every point M is the same matrix inside a voxel and the translation part, -sum n_v M sum_i (mean_v - p_i), is zero by the definition of
    the mean; what is left is FP64 rounding of sums of ~n terms of size |M| |e|."""
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-5, 5, (2000, 3)).astype(np.float32)
    c = np.repeat(np.diag([0.02, 0.01, 0.03])[None], 2000, 0)
    g = vm.VoxelGICPModel(tgt, tgt, c, c, 1.0)
    H, b, err = g.linearize(np.eye(4))
    assert (g.corr >= 0).all() and (g.vmap.ijk[g.corr] == vm.voxel_of(tgt, 1.0)).all()
    scale = float((g.vmap.count[g.corr] * np.abs(np.linalg.inv(2 * c[0])).max() * np.abs(g.vmap.mean[g.corr] - tgt).max(1)).sum())
    print("translation gradient", np.abs(b[3:]).max(), "of a sum of magnitude", scale)
    assert np.abs(b[3:]).max() <= 1e-13 * scale
    assert err > 0


def test_points_outside_every_voxel_contribute_nothing():
    g = _scene()
    far = np.r_[g.src, np.array([[100, 100, 100], [np.nan, 0, 0], [3e7, 0, 0]], np.float32)]
    cs = np.r_[vm.cov3(g.ca), np.repeat(np.eye(3)[None], 3, 0)]
    g2 = vm.VoxelGICPModel(far, g.tgt, cs, g.cb, 1.0)
    T = clouds.make_pose((0.05, -0.02, 0.03), (0.5, -0.4, 0.8))
    H, b, e = g.linearize(T)
    H2, b2, e2 = g2.linearize(T)
    assert (g2.corr[-3:] == -1).all() and np.isinf(g2.sqd[-3:]).all()
    assert np.array_equal(H, H2) and np.array_equal(b, b2) and e == e2


# ---- the loop -------------------------------------------------------------------------------------------------------------------
def test_the_lm_loop_moves_towards_the_ground_truth():
    """3k -> 6k (two keyframes), 1 m voxels, NumpyGICP.align's loop."""
    w = clouds.scan_to_submap(3008, 2)
    assert w.source.shape[0] == 3008 and w.target.shape[0] == 6016
    g = vm.VoxelGICPModel(w.source, w.target, vm.plane_covariances(w.source), vm.plane_covariances(w.target), 1.0, max_iter=32, trans_eps=1e-3)
    T = g.align(w.guess)
    start, end = clouds.pose_error(w.guess, w.gt), clouds.pose_error(T, w.gt)
    print("start", start, "end", end, "iterations", g.nr_iterations + 1, "voxels", len(g.vmap))
    # measured when written: start (0.0616 m, 0.0108 rad) -> end (0.0028 m, 0.00012 rad) after 3 iterations over 2364 voxels; that is a
    # record, not a bound: the assertion is "nearer"
    assert end[0] < start[0] and end[1] < start[1]


# ---- the declared ABI -----------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entries():
    hdr = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    from direct_lidar_odometry_amd import nano_gicp
    for name in ("ngicp_set_voxel_resolution", "ngicp_voxelmap_size", "ngicp_voxelmap_get"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in nano_gicp.EXPORTS
    for m in ("setVoxelResolution", "getVoxelResolution", "getVoxelMapSize", "voxelMap"):
        assert hasattr(nano_gicp.NanoGICP, m)
    shim = open(os.path.join(ROOT, "include", "nano_gicp", "nano_gicp.hpp")).read()
    for m in ("setVoxelResolution", "getVoxelResolution", "getVoxelMapSize"):
        assert m in shim
