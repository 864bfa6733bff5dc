"""Independent numpy (float64) model of voxelized GICP as include/ngicp.h defines it ("voxelized GICP").   *** TEST INFRASTRUCTURE ONLY ***

The definition is the project's own, so the model is checked against itself (tests/test_vgicp_model_cpu.py: symmetry, finite
differences, a cloud on its own map) and the engine against the model (tests/test_gpu_vgicp.py).  The float32 parts - the voxel of a
point, the float pose times the point - are spelled operation by operation, as oracle/numpy_model.py spells the transform: numpy
rounds every float32 operation to float32, nothing is fused.  Everything else is float64.
Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

from oracle.numpy_model import NumpyGICP  # the LM loop (NumpyGICP.align) is reused unchanged

VOXEL_LIMIT = 1 << 20  # |i| < 2^20 on every axis


def voxel_of(p, res) -> np.ndarray:
    """ijk = floorf(p * inv_res) per axis, inv_res = 1.0f / (float)res: one float32 multiply, then floor.  (N, 3) int64."""
    inv = np.float32(1.0) / np.float32(res)
    q = np.floor(np.asarray(p, np.float32) * inv)  # float32 * float32 -> float32
    return np.where(np.isfinite(q), q, np.float32(2.0 ** 40)).astype(np.int64)  # (a non-finite coordinate: beyond every limit)


def transform_f32(T, pts) -> np.ndarray:
    """float(T) * point in the engine's order, ((c0*x + c1*y) + c2*z) + c3, every operation rounded to float32."""
    Tf = np.asarray(T, np.float32)
    p = np.asarray(pts, np.float32)
    return np.stack([((Tf[r, 0] * p[:, 0] + Tf[r, 1] * p[:, 1]) + Tf[r, 2] * p[:, 2]) + Tf[r, 3] for r in range(3)], axis=1)


def cov3(c) -> np.ndarray:
    """(N, 4, 4) or (N, 3, 3) covariances -> (N, 3, 3) float64."""
    return np.asarray(c, np.float64)[:, :3, :3]


class VoxelMap:
    """Per occupied voxel, in ascending (iz, iy, ix): ijk, count, mean = (sum (double)p) / n, cov = (sum C) / n, every sum taken one
    term after the other in ascending original target index."""

    def __init__(self, target, covs, res):
        tgt = np.asarray(target, np.float32)
        C = cov3(covs)
        ijk = voxel_of(tgt, res)
        if not np.isfinite(tgt).all() or (np.abs(ijk) >= VOXEL_LIMIT).any():
            raise ValueError("a target point lies 2^20 voxels or more from the origin")
        order = np.lexsort((np.arange(len(tgt)), ijk[:, 0], ijk[:, 1], ijk[:, 2]))  # primary iz, then iy, ix, then the original index
        s = ijk[order]
        head = np.r_[True, (s[1:] != s[:-1]).any(axis=1)]
        starts = np.flatnonzero(head)
        ends = np.r_[starts[1:], len(tgt)]
        self.res = res
        self.ijk = s[starts]
        self.count = (ends - starts).astype(np.int64)
        self.mean = np.empty((len(starts), 3))
        self.cov = np.empty((len(starts), 3, 3))
        self.members = []
        p64 = tgt.astype(np.float64)
        for v, (a, b) in enumerate(zip(starts, ends)):
            idx = order[a:b]
            m, c = np.zeros(3), np.zeros((3, 3))
            for j in idx:  # one after the other: the order of the sum is part of the definition
                m = m + p64[j]
                c = c + C[j]
            self.mean[v] = m / (b - a)
            self.cov[v] = c / (b - a)
            self.members.append(idx)
        self._index = {tuple(k): v for v, k in enumerate(self.ijk.tolist())}

    def __len__(self):
        return len(self.ijk)

    def lookup(self, q_f32) -> np.ndarray:
        """voxel number of every float32 point, -1 where its voxel is empty (or out of range)."""
        ijk = voxel_of(q_f32, self.res)
        ok = np.isfinite(np.asarray(q_f32, np.float32)).all(axis=1) & (np.abs(ijk) < VOXEL_LIMIT).all(axis=1)
        return np.array([self._index.get(tuple(k), -1) if o else -1 for k, o in zip(ijk.tolist(), ok)], dtype=np.int64)


def terms(src, cov_src, vmap, corr, T, weight=None, T_eval=None):
    """(H, b, err) over the source points with corr >= 0: e = mean_v - T_eval a, M = (cov_v + R C_a R^T)^-1 with R of T,
    J = [skew(T_eval a) | -I]; err += n_v e^T M e, H += n_v J^T M J, b += n_v J^T M e.  weight: the frozen n_v M of an earlier
    linearisation (compute_error evaluates a trial pose under the matrices of the last linearisation)."""
    T = np.asarray(T, np.float64)
    T_eval = T if T_eval is None else np.asarray(T_eval, np.float64)
    rows = np.flatnonzero(corr >= 0)
    if len(rows) == 0:
        return np.zeros((6, 6)), np.zeros(6), 0.0, np.zeros((len(corr), 3, 3))
    v = corr[rows]
    if weight is None:
        R = T[:3, :3]
        M = np.linalg.inv(vmap.cov[v] + R @ cov3(cov_src)[rows] @ R.T)
        W = vmap.count[v][:, None, None] * M
    else:
        W = weight[rows]
    ta = np.asarray(src, np.float64)[rows] @ T_eval[:3, :3].T + T_eval[:3, 3]
    e = vmap.mean[v] - ta
    J = np.zeros((len(rows), 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0] = -ta[:, 2], ta[:, 1], ta[:, 2]
    J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = -ta[:, 0], -ta[:, 1], ta[:, 0]
    J[:, :, 3:] = -np.eye(3)
    H = np.einsum("nri,nrs,nsj->ij", J, W, J)
    b = np.einsum("nri,nrs,ns->i", J, W, e)
    err = float(np.einsum("ni,nij,nj->", e, W, e))
    full = np.zeros((len(corr), 3, 3))
    full[rows] = W
    return H, b, err, full


class VoxelGICPModel(NumpyGICP):
    """NumpyGICP with the correspondence rule and the terms of voxelized GICP; align() is NumpyGICP.align, untouched.
    max_corr_dist is accepted and never consulted (voxel membership is the gate)."""

    def __init__(self, source, target, cov_src, cov_tgt, res, **kw):
        super().__init__(source, target, cov_src, cov_tgt, **kw)
        self.vmap = VoxelMap(self.tgt, cov_tgt, res)

    def update_correspondences(self, T):  # DIRECT1: the voxel of float(T) * a, if occupied
        self.q = transform_f32(np.asarray(T, np.float64).astype(np.float32), self.src)
        self.corr = self.vmap.lookup(self.q)
        m = np.where(self.corr >= 0, self.corr, 0)
        d = self.q - self.vmap.mean[m].astype(np.float32)
        self.sqd = np.where(self.corr >= 0, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], np.float32(np.inf)).astype(np.float32)
        self.weight = None

    def accumulate(self, T, want=True):
        T = np.asarray(T, np.float64)
        if want:  # a linearisation: the matrices are those of this pose, and stay for the trials
            H, b, err, self.weight = terms(self.src, self.ca, self.vmap, self.corr, T)
            return H, b, err
        H, b, err, _ = terms(self.src, self.ca, self.vmap, self.corr, T, weight=self.weight)
        return H, b, err

    def compute_error(self, T):
        return self.accumulate(T, want=False)[2]


def plane_covariances(pts, k=20) -> np.ndarray:
    """PLANE-regularised k-NN covariances (N, 4, 4), vectorised: eigenvalues replaced by (1e-3, 1, 1) along the eigenvectors of the
    neighbourhood's covariance.  Any symmetric positive definite set would do for the model's tests; this one has the shape of the
    engine's default."""
    p = np.asarray(pts, np.float64)
    n = len(p)
    out = np.zeros((n, 4, 4))
    for lo in range(0, n, 512):
        blk = p[lo:lo + 512]
        d2 = ((blk[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        idx = np.argpartition(d2, k - 1, axis=1)[:, :k]
        nb = p[idx]
        nb = nb - nb.mean(axis=1, keepdims=True)
        c = np.einsum("nki,nkj->nij", nb, nb) / k
        _, V = np.linalg.eigh(c)  # ascending eigenvalues
        out[lo:lo + 512, :3, :3] = np.einsum("nij,j,nkj->nik", V, np.array([1e-3, 1.0, 1.0]), V)
    return out
