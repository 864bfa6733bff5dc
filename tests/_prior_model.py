"""The numpy model of the pose prior (include/ngicp.h, "pose prior") on top of the project's models: tests/_robust_model.py's exact and
voxelized classes (which are the plain ones with the kernel NONE).   *** TEST INFRASTRUCTURE ONLY ***

The definition is the project's own, so the model proves itself (tests/test_prior_model_cpu.py) and the engine is held to the model
(tests/test_gpu_pose_prior.py).  `_Prior.accumulate` adds the prior's row to what the parent's accumulate returns; correspondences,
matrices, the robust kernel and NumpyGICP.align (the LM loop) are the parents', untouched.  Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

import _robust_model as rm
import _vgicp_model as vm
from oracle.numpy_model import NumpyGICP, skew, so3_exp

LOG_TAYLOR_S2 = 1e-6    # so3_log: the series below |sin(theta) axis|^2 = 1e-6, atan2 from there
JINV_TAYLOR_TH2 = 1e-2  # jinv_coeff: the series below theta^2 = 1e-2, the half-angle form from there


def so3_log(R):
    """The inverse of so3_exp for rotation angles up to 3 rad: v = (R - R^T)^vee / 2 = sin(theta) axis, c = cos(theta)."""
    R = np.asarray(R, np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = 0.5 * ((R[0, 0] + R[1, 1] + R[2, 2]) - 1.0)
    s2 = float(v @ v)
    if s2 < LOG_TAYLOR_S2 and c > 0.0:
        f = 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0 + s2 * (15.0 / 336.0)))
    else:
        s = np.sqrt(s2)
        f = np.arctan2(s, c) / s if s > 0.0 else 0.0
    return f * v


def jinv_coeff(th2):
    if th2 < JINV_TAYLOR_TH2:
        return 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0 + th2 * (1.0 / 1209600.0 + th2 * (1.0 / 47900160.0))))
    half = 0.5 * np.sqrt(th2)
    return (1.0 - half * np.cos(half) / np.sin(half)) / th2


def left_jacobian_inv(phi):
    """J_l^{-1}(phi) = I - [phi]x / 2 + k [phi]x^2, with [phi]x^2 = phi phi^T - |phi|^2 I"""
    phi = np.asarray(phi, np.float64)
    th2 = float(phi @ phi)
    return (np.eye(3) - 0.5 * skew(phi)) + jinv_coeff(th2) * (np.outer(phi, phi) - th2 * np.eye(3))


def residual(T, Tp):
    T, Tp = np.asarray(T, np.float64), np.asarray(Tp, np.float64)
    return np.r_[so3_log(T[:3, :3] @ Tp[:3, :3].T), T[:3, 3] - Tp[:3, 3]]


def jacobian(T, r):
    """d r / d d under T <- (so3_exp(d[0:3]), d[3:6]) * T"""
    J = np.zeros((6, 6))
    J[:3, :3] = left_jacobian_inv(r[:3])
    J[3:, :3] = -skew(np.asarray(T, np.float64)[:3, 3])
    J[3:, 3:] = np.eye(3)
    return J


def prior_terms(T, Tp, Lam):
    """-> (r, r^T L r, J_p^T L J_p, J_p^T L r): every sum is u^T (L w)"""
    Lam = np.asarray(Lam, np.float64)
    r = residual(T, Tp)
    J = jacobian(T, r)
    return r, float(r @ (Lam @ r)), J.T @ (Lam @ J), J.T @ (Lam @ r)


def prior_row(T, Tp, Lam):
    """The 28 sums of the device's prior_row: H's upper triangle row by row, b, the cost."""
    _, c, H, b = prior_terms(T, Tp, Lam)
    return np.r_[H[np.triu_indices(6)], b, c]


def left_update(d, T):
    """(so3_exp(d[0:3]), d[3:6]) * T"""
    D = np.eye(4)
    D[:3, :3] = so3_exp(np.asarray(d[:3], np.float64))
    D[:3, 3] = d[3:]
    return D @ np.asarray(T, np.float64)


class _Prior:
    prior = None

    def set_prior(self, Tp, Lam):
        self.prior = None if Tp is None else (np.asarray(Tp, np.float64).copy(), np.asarray(Lam, np.float64).copy())
        return self

    def accumulate(self, T, want=True):
        H, b, err = super().accumulate(T, want)
        if self.prior is None:
            return H, b, err
        _, c, Hp, bp = prior_terms(T, *self.prior)
        return H + Hp, b + bp, err + c


class PriorNumpyGICP(_Prior, rm.RobustNumpyGICP):
    """Exact GICP with an optional robust kernel and an optional prior."""


class PriorVoxelGICPNbrModel(_Prior, rm.RobustVoxelGICPNbrModel):
    """DIRECT1 / 7 / 27 likewise."""


def make_model(K, src, tgt, cs, ct, res=1.0, vmap=None, **kw):
    """K = 0: exact GICP; 1, 7, 27: the voxelized neighbourhoods on `vmap` (built from the target when None)."""
    if K == 0:
        return PriorNumpyGICP(src, tgt, cs, ct, **kw)
    m = PriorVoxelGICPNbrModel.__new__(PriorVoxelGICPNbrModel)
    NumpyGICP.__init__(m, src, tgt, cs, ct, **kw)
    m.vmap = vm.VoxelMap(m.tgt, ct, res) if vmap is None else vmap
    m.set_neighbors(K)
    return m


def corridor(n=600, seed=3, length=12.0, half_width=1.5, height=2.5, noise=0.01):
    """A corridor along x: a floor and two walls, no end walls, `noise` m of Gaussian noise on every coordinate.  Float32 (n, 3)."""
    rng = np.random.default_rng(seed)
    k = n // 3
    x = rng.uniform(-0.5 * length, 0.5 * length, n)
    floor = np.c_[x[:k], rng.uniform(-half_width, half_width, k), np.zeros(k)]
    left = np.c_[x[k:2 * k], np.full(k, half_width), rng.uniform(0, height, k)]
    right = np.c_[x[2 * k:], np.full(n - 2 * k, -half_width), rng.uniform(0, height, n - 2 * k)]
    return np.ascontiguousarray((np.r_[floor, left, right] + rng.normal(0, noise, (n, 3))).astype(np.float32))


def corridor_case(n=900, shift=0.5, guess_off=0.3, noise=0.01, seed=5):
    """-> dict: a scan of the corridor; the target, a copy of the corridor displaced by `shift` along the axis, sampled at points of its
    own and over a longer stretch (so that neither point identities nor the ends of the clouds tell where along the axis the scan lies:
    ground truth, source -> target, is that translation); the guess `guess_off` further along the axis; covariances of both clouds from
    the model's side (vm.plane_covariances).  The defaults are the case tests/test_prior_model_cpu.py records."""
    src = corridor(n, seed=seed, noise=noise)
    gt = np.eye(4)
    gt[0, 3] = shift
    tgt = np.ascontiguousarray((corridor(2 * n, seed=seed + 14, length=24.0, noise=noise).astype(np.float64) + gt[:3, 3]).astype(np.float32))
    guess = gt.copy()
    guess[0, 3] += guess_off
    return dict(src=src, tgt=tgt, gt=gt, guess=guess.astype(np.float32), cs=vm.plane_covariances(src, 20), ct=vm.plane_covariances(tgt, 20))


def axis_prior(T_true, weight):
    """An axis-only prior at the true pose: information `weight` (m^-2) on the translation along x, nothing else."""
    Lam = np.zeros((6, 6))
    Lam[3, 3] = weight
    return np.asarray(T_true, np.float64), Lam
