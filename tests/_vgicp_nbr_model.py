"""The numpy model of voxelized GICP's neighbourhoods (include/ngicp.h, "voxelized GICP": NGICP_VOX_DIRECT1 / 7 / 27) on top of
tests/_vgicp_model.py.   *** TEST INFRASTRUCTURE ONLY ***

A neighbourhood is a fixed, ordered list of K integer voxel offsets; slot s of a source point whose voxel is c corresponds to voxel
c + off[s] if c is in range, c + off[s] is in range on every axis (tested on the integers) and that voxel is occupied.  The terms of every
occupied slot are _vgicp_model.terms' and are summed.  The model proves itself in tests/test_vgicp_nbr_model_cpu.py; the engine is held
to it in tests/test_gpu_vgicp_nbr.py.  Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

import _vgicp_model as vm

# (dx, dy, dz) per slot, spelled out
OFFSETS = {
    1: ((0, 0, 0),),
    7: ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)),
    27: ((-1, -1, -1), (0, -1, -1), (1, -1, -1), (-1, 0, -1), (0, 0, -1), (1, 0, -1), (-1, 1, -1), (0, 1, -1), (1, 1, -1),
         (-1, -1, 0), (0, -1, 0), (1, -1, 0), (-1, 0, 0), (0, 0, 0), (1, 0, 0), (-1, 1, 0), (0, 1, 0), (1, 1, 0),
         (-1, -1, 1), (0, -1, 1), (1, -1, 1), (-1, 0, 1), (0, 0, 1), (1, 0, 1), (-1, 1, 1), (0, 1, 1), (1, 1, 1)),
}
CENTRE = {1: 0, 7: 0, 27: 13}


def lookup_slots(vmap, q_f32, K) -> np.ndarray:
    """(n, K) voxel numbers of the float32 points q under neighbourhood K, -1 where a slot has no voxel."""
    q = np.asarray(q_f32, np.float32)
    c = vm.voxel_of(q, vmap.res)  # int64: the range tests below are on integers
    centre_ok = np.isfinite(q).all(axis=1) & (np.abs(c) < vm.VOXEL_LIMIT).all(axis=1)
    out = np.full((len(q), K), -1, dtype=np.int64)
    for s, off in enumerate(OFFSETS[K]):
        nb = c + np.asarray(off, np.int64)
        ok = centre_ok & (np.abs(nb) < vm.VOXEL_LIMIT).all(axis=1)
        out[:, s] = [vmap._index.get(tuple(k), -1) if o else -1 for k, o in zip(nb.tolist(), ok)]
    return out


class VoxelGICPNbrModel(vm.VoxelGICPModel):
    """VoxelGICPModel with a neighbourhood: corr_n is (n, K); corr / sqd stay the CENTRE slot's (what ngicp_get_correspondences
    reports).  align() is NumpyGICP.align, untouched."""

    def __init__(self, source, target, cov_src, cov_tgt, res, neighbors=1, **kw):
        super().__init__(source, target, cov_src, cov_tgt, res, **kw)
        self.set_neighbors(neighbors)

    def set_neighbors(self, K):
        assert K in OFFSETS
        self.K = K
        self.corr_n = None
        self.weight = None

    def update_correspondences(self, T):
        self.q = vm.transform_f32(np.asarray(T, np.float64).astype(np.float32), self.src)
        self.corr_n = lookup_slots(self.vmap, self.q, self.K)
        self.corr = self.corr_n[:, CENTRE[self.K]].copy()
        m = np.where(self.corr >= 0, self.corr, 0)
        d = self.q - self.vmap.mean[m].astype(np.float32)
        self.sqd = np.where(self.corr >= 0, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], np.float32(np.inf)).astype(np.float32)
        self.weight = None
        self.T_lin = None

    def accumulate(self, T, want=True):
        T = np.asarray(T, np.float64)
        if want:  # a linearisation: the K sets of matrices are those of this pose, and stay for the trials
            parts = [vm.terms(self.src, self.ca, self.vmap, self.corr_n[:, s], T) for s in range(self.K)]
            self.weight = [p[3] for p in parts]
            self.T_lin = T.copy()
        else:
            parts = [vm.terms(self.src, self.ca, self.vmap, self.corr_n[:, s], T, weight=self.weight[s]) for s in range(self.K)]
        H, b, err = parts[0][:3]
        for p in parts[1:]:  # ascending slot
            H, b, err = H + p[0], b + p[1], err + p[2]
        return H, b, err


def slab(seed=5):
    """The case that separates the modes: a thin wall inside the voxels ix = 0 and a source one whole voxel in front of it."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(0, 6, (600, 3)).astype(np.float32)
    tgt[:, 0] = rng.uniform(0.02, 0.1, 600).astype(np.float32)
    src = tgt[:257].copy()
    src[:, 0] += np.float32(1.0)
    A = rng.normal(0, 0.1, (600, 3, 3))
    ct = np.zeros((600, 4, 4))
    ct[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    cs = ct[:257].copy()
    return src, tgt, cs, ct
