"""The numpy model of the robust kernels (include/ngicp.h, "robust kernel") on top of the project's three models: oracle/numpy_model.py
(exact GICP), tests/_vgicp_model.py (DIRECT1) and tests/_vgicp_nbr_model.py (DIRECT7 / DIRECT27).   *** TEST INFRASTRUCTURE ONLY ***

The definition is the project's own, so the model proves itself (tests/test_robust_model_cpu.py) and the engine is held to the model
(tests/test_gpu_robust.py).  Every subclass overrides `accumulate` alone: correspondences, matrices and NumpyGICP.align (the LM loop)
are the parents', untouched.  After an accumulate, `last_s` / `last_w` hold the per-term s and w as (n, K) arrays with the engine's
markers (-1 / 0 where a slot has no correspondence).  Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

import _vgicp_model as vm
import _vgicp_nbr_model as nbm
from oracle.numpy_model import NumpyGICP

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3
KINDS = (HUBER, CAUCHY, GEMAN_MCCLURE)
NAMES = {NONE: "none", HUBER: "huber", CAUCHY: "cauchy", GEMAN_MCCLURE: "geman_mcclure"}


def rho_w(s, kind, c):
    """rho(s) and w(s) = d rho / d s of every entry of s; an entry with !(s > 0) passes through as under NONE."""
    s = np.asarray(s, np.float64)
    rho, w = s.copy(), np.ones_like(s)
    c = float(c)
    c2 = c * c
    ok = s > 0
    with np.errstate(over="ignore"):
        if kind == HUBER:
            o = ok & ~(s <= c2)
            r = np.sqrt(s[o])
            rho[o] = 2.0 * c * r - c2
            w[o] = c / r
        elif kind == CAUCHY:
            u = s[ok] / c2
            rho[ok] = c2 * np.log1p(u)
            w[ok] = 1.0 / (1.0 + u)
        elif kind == GEMAN_MCCLURE:
            q = c2 / (c2 + s[ok])
            rho[ok] = s[ok] * q
            w[ok] = q * q
        elif kind != NONE:
            raise ValueError(f"unknown robust kernel {kind}")
    return rho, w


def jacobians(ta):
    """J = [skew(T a) | -I] per row of ta: (n, 3, 6)."""
    J = np.zeros((len(ta), 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0] = -ta[:, 2], ta[:, 1], ta[:, 2]
    J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = -ta[:, 0], -ta[:, 1], ta[:, 0]
    J[:, :, 3:] = -np.eye(3)
    return J


def weighted_sums(ta, e, M, kind, c):
    """(H, b, sum rho, s, w) of the terms with residuals e, matrices M (n, 3, 3) and transformed source points ta."""
    s = np.einsum("ni,nij,nj->n", e, M, e)
    rho, w = rho_w(s, kind, c)
    J = jacobians(ta)
    Mw = M * w[:, None, None]
    return np.einsum("nri,nrs,nsj->ij", J, Mw, J), np.einsum("nri,nrs,ns->i", J, Mw, e), float(rho.sum()), s, w


class _Robust:
    kind, width = NONE, 1.0

    def set_kernel(self, kind, width=1.0):
        self.kind, self.width = int(kind), float(width)
        return self

    def compute_error(self, T):  # (NumpyGICP has none of its own; the voxel models' is this very line)
        return self.accumulate(T, want=False)[2]

    def _slot(self, rows, ta, e, M, n, out_s, out_w, slot):
        H, b, err, s, w = weighted_sums(ta, e, M, self.kind, self.width)
        out_s[rows, slot], out_w[rows, slot] = s, w
        return H, b, err


class RobustNumpyGICP(_Robust, NumpyGICP):
    """Exact GICP: one term per source point with a correspondence; the matrices are self.mahal (update_correspondences')."""

    def accumulate(self, T, want=True):
        T = np.asarray(T, np.float64)
        n = len(self.src)
        self.last_s, self.last_w = np.full((n, 1), -1.0), np.zeros((n, 1))
        rows = np.flatnonzero(self.corr >= 0)
        if len(rows) == 0:
            return np.zeros((6, 6)), np.zeros(6), 0.0
        ta = self.src[rows].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        e = self.tgt[self.corr[rows]].astype(np.float64) - ta
        return self._slot(rows, ta, e, self.mahal[rows][:, :3, :3], n, self.last_s, self.last_w, 0)


def _voxel_accumulate(m, corr_slots, T, want):
    """The voxelized terms of the (n, K) voxel numbers corr_slots: a linearisation computes and keeps n_v M per slot (m.weight, a list
    of K (n, 3, 3) arrays), a trial reuses it.  Slots are added in ascending order."""
    T = np.asarray(T, np.float64)
    n, K = corr_slots.shape
    m.last_s, m.last_w = np.full((n, K), -1.0), np.zeros((n, K))
    if want:
        m.weight = [np.zeros((n, 3, 3)) for _ in range(K)]
    H, b, err = np.zeros((6, 6)), np.zeros(6), 0.0
    for s in range(K):
        rows = np.flatnonzero(corr_slots[:, s] >= 0)
        if len(rows) == 0:
            continue
        v = corr_slots[rows, s]
        if want:
            R = T[:3, :3]
            m.weight[s][rows] = m.vmap.count[v][:, None, None] * np.linalg.inv(m.vmap.cov[v] + R @ vm.cov3(m.ca)[rows] @ R.T)
        ta = m.src[rows].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        p = m._slot(rows, ta, m.vmap.mean[v] - ta, m.weight[s][rows], n, m.last_s, m.last_w, s)
        H, b, err = H + p[0], b + p[1], err + p[2]
    return H, b, err


class RobustVoxelGICPModel(_Robust, vm.VoxelGICPModel):
    """DIRECT1: one term per source point whose voxel is occupied."""

    def accumulate(self, T, want=True):
        return _voxel_accumulate(self, self.corr[:, None], T, want)


class RobustVoxelGICPNbrModel(_Robust, nbm.VoxelGICPNbrModel):
    """DIRECT1 / 7 / 27: up to K terms per source point."""

    def accumulate(self, T, want=True):
        if want:
            self.T_lin = np.asarray(T, np.float64).copy()
        return _voxel_accumulate(self, self.corr_n, T, want)


def outlier_scenario(w, shift=(0.35, 0.25, 0.0), lo=0.2, span=np.pi / 3):
    """The workload's source with the points whose azimuth lies in (lo, lo + span) shifted: (source, mask of the shifted points)."""
    src = np.array(w.source, np.float32, copy=True)
    az = np.arctan2(src[:, 1], src[:, 0])
    sel = (az > lo) & (az < lo + span)
    src[sel] += np.float32(shift)
    return np.ascontiguousarray(src), sel
