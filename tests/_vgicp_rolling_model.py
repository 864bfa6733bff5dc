"""Independent numpy (float64) model of the rolling voxel map as include/ngicp.h defines it ("rolling voxel map").   *** TEST INFRASTRUCTURE ONLY ***

A dict keyed by ijk holds, per voxel, the sums S (3), C (3x3), the count and the stamp; a list keeps the order of first insertion, which
is the numbering.  Every sum is taken term by term in the stated order, the float32 transform and the rotation of a covariance sum are
spelled operation by operation (numpy rounds every operation to its type, nothing is fused).  RollingVoxelMap offers what
_vgicp_model.VoxelMap offers (ijk, count, mean, cov, __len__, lookup), so VoxelGICPModel / VoxelGICPNbrModel run on it unchanged.
Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

from _vgicp_model import VOXEL_LIMIT, cov3, voxel_of


def transform_pcl_f32(T, pts) -> np.ndarray:
    """float(T) * point in the order of pcl::transformPointCloud as the engine restates it (csrc/ngicp_cloudops.h transform_point_f):
    x*c0 + (y*c1 + (z*c2 + c3)), every operation rounded to float32."""
    Tf = np.asarray(T, np.float32)
    p = np.asarray(pts, np.float32)
    with np.errstate(all="ignore"):
        return np.stack([p[:, 0] * Tf[r, 0] + (p[:, 1] * Tf[r, 1] + (p[:, 2] * Tf[r, 2] + Tf[r, 3])) for r in range(3)], axis=1)


def rotate_sym(R, A) -> np.ndarray:
    """R A R^T of a symmetric 3x3 in the engine's order (csrc/ngicp_math.h rotate_sym): RA = R A row by row, each entry
    (r0*a0 + r1*a1) + r2*a2; then the six entries of the upper triangle of RA R^T the same way.  Returns the full symmetric matrix."""
    R = np.asarray(R, np.float64)
    a = np.asarray(A, np.float64)
    a00, a01, a02, a11, a12, a22 = a[0, 0], a[0, 1], a[0, 2], a[1, 1], a[1, 2], a[2, 2]
    RA = np.empty((3, 3))
    for r in range(3):
        r0, r1, r2 = R[r]
        RA[r, 0] = r0 * a00 + r1 * a01 + r2 * a02
        RA[r, 1] = r0 * a01 + r1 * a11 + r2 * a12
        RA[r, 2] = r0 * a02 + r1 * a12 + r2 * a22
    o = np.empty((3, 3))
    for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        o[i, j] = o[j, i] = RA[i, 0] * R[j, 0] + RA[i, 1] * R[j, 1] + RA[i, 2] * R[j, 2]
    return o


class Refused(ValueError):
    """an insert with a transformed point that has no voxel"""


class RollingVoxelMap:
    def __init__(self, res):
        self.res = res
        self.inserts = 0
        self._acc = {}    # (ix, iy, iz) -> [S (3), C (3, 3), n, stamp]
        self._order = []  # keys in order of first insertion: the numbering
        self._refresh()

    # ---- the definition ----
    def scan_sums(self, points, covs, T):
        """The scan's own per-voxel sums at the float pose T: {key: (s, c, n)} and the keys in ascending (iz, iy, ix).  Raises Refused
        when a transformed point has no voxel."""
        Tf = np.asarray(T, np.float32)
        q = transform_pcl_f32(Tf, points)
        ijk = voxel_of(q, self.res)
        if not np.isfinite(q).all() or (np.abs(ijk) >= VOXEL_LIMIT).any():
            raise Refused("a transformed point lies 2^20 voxels or more from the origin (or is not finite)")
        C = cov3(covs)
        R = Tf[:3, :3].astype(np.float64)
        q64 = q.astype(np.float64)
        groups = {}
        for j, key in enumerate(map(tuple, ijk.tolist())):  # ascending original index
            groups.setdefault(key, []).append(j)
        out = {}
        for key, idx in groups.items():
            s, c = np.zeros(3), np.zeros((3, 3))
            for j in idx:  # one after the other: the order of the sum is part of the definition
                s = s + q64[j]
                c = c + C[j]
            out[key] = (s, rotate_sym(R, c), len(idx))  # ONE rotation per voxel, applied to the sum
        return out, sorted(out, key=lambda k: (k[2], k[1], k[0]))

    def insert(self, points, covs, T):
        """-> (voxels created, voxels of the scan).  A refused insert raises before anything is written."""
        sums, keys = self.scan_sums(points, covs, T)
        stamp = self.inserts + 1
        n_new = 0
        for key in keys:  # new voxels are numbered in ascending (iz, iy, ix)
            s, c, n = sums[key]
            if key in self._acc:
                a = self._acc[key]
                a[0] = a[0] + s
                a[1] = a[1] + c
                a[2] += n
                a[3] = stamp
            else:
                self._acc[key] = [s.copy(), c.copy(), n, stamp]
                self._order.append(key)
                n_new += 1
        self.inserts = stamp
        self._refresh()
        return n_new, len(keys)

    def evict(self, centre=(0.0, 0.0, 0.0), max_dist=0.0, min_stamp=0):
        """-> voxels removed; survivors keep their relative order."""
        c = np.asarray(centre, np.float32).astype(np.float64)
        res, md = np.float64(self.res), np.float64(max_dist)
        keep = []
        for key in self._order:
            gone = False
            if md > 0:
                d = (np.array(key, np.float64) + 0.5) * res - c
                gone = bool(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > md * md)
            if min_stamp > 0 and self._acc[key][3] < min_stamp:
                gone = True
            if gone:
                del self._acc[key]
            else:
                keep.append(key)
        removed = len(self._order) - len(keep)
        self._order = keep
        self._refresh()
        return removed

    def clear(self):
        self._acc.clear()
        self._order = []
        self.inserts = 0
        self._refresh()

    # ---- the vmap interface of the other models ----
    def _refresh(self):
        k = self._order
        n = len(k)
        self.ijk = np.array(k, dtype=np.int64).reshape(n, 3)
        self.count = np.array([self._acc[x][2] for x in k], dtype=np.int64)
        self.stamp = np.array([self._acc[x][3] for x in k], dtype=np.int64)
        self.sum = np.array([self._acc[x][0] for x in k]).reshape(n, 3)
        self.covsum = np.array([self._acc[x][1] for x in k]).reshape(n, 3, 3)
        self.mean = np.array([self._acc[x][0] / float(self._acc[x][2]) for x in k]).reshape(n, 3)
        self.cov = np.array([self._acc[x][1] / float(self._acc[x][2]) for x in k]).reshape(n, 3, 3)
        self._index = {x: v for v, x in enumerate(k)}

    def __len__(self):
        return len(self._order)

    def lookup(self, q_f32) -> np.ndarray:
        """voxel number of every float32 point, -1 where its voxel is empty (or out of range)."""
        ijk = voxel_of(q_f32, self.res)
        ok = np.isfinite(np.asarray(q_f32, np.float32)).all(axis=1) & (np.abs(ijk) < VOXEL_LIMIT).all(axis=1)
        return np.array([self._index.get(tuple(k), -1) if o else -1 for k, o in zip(ijk.tolist(), ok)], dtype=np.int64)

    def snapshot(self):
        """everything that must not change under a refused insert, as one comparable tuple of bytes"""
        return (self.inserts, self.ijk.tobytes(), self.count.tobytes(), self.stamp.tobytes(), self.sum.tobytes(), self.covsum.tobytes())
