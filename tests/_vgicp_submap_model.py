"""Independent numpy (float64) model of the merged voxel map as include/ngicp.h defines it ("merged voxel map").   *** TEST INFRASTRUCTURE ONLY ***

Two definitions are restated: the voxel part of one keyframe (per-voxel sums, no division) and the map merged from the parts of a list of
keyframes.  Every sum is taken term by term in the stated order, as _vgicp_model.VoxelMap takes its own.  MergedVoxelMap offers what
VoxelMap offers (ijk, count, mean, cov, lookup), so VoxelGICPModel runs on it unchanged.
Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

from _vgicp_model import VOXEL_LIMIT, cov3, voxel_of


class VoxelPart:
    """One keyframe's per-voxel sums at resolution `res`: for every voxel that holds a point, n, s = sum (double)p (3) and c = sum C (3x3),
    each sum started at 0.0 and added in ascending original index inside the keyframe; voxels in ascending (iz, iy, ix); no division."""

    def __init__(self, points, covs, res):
        pts = np.asarray(points, np.float32)
        C = cov3(covs)
        ijk = voxel_of(pts, res)
        if not np.isfinite(pts).all() or (np.abs(ijk) >= VOXEL_LIMIT).any():
            raise ValueError("a keyframe point lies 2^20 voxels or more from the origin")
        order = np.lexsort((np.arange(len(pts)), ijk[:, 0], ijk[:, 1], ijk[:, 2]))
        s = ijk[order]
        head = np.r_[True, (s[1:] != s[:-1]).any(axis=1)]
        starts = np.flatnonzero(head)
        ends = np.r_[starts[1:], len(pts)]
        self.res = res
        self.ijk = s[starts]
        self.count = (ends - starts).astype(np.int64)
        self.sum = np.empty((len(starts), 3))
        self.covsum = np.empty((len(starts), 3, 3))
        p64 = pts.astype(np.float64)
        for v, (a, b) in enumerate(zip(starts, ends)):
            m, c = np.zeros(3), np.zeros((3, 3))
            for j in order[a:b]:  # one after the other: the order of the sum is part of the definition
                m = m + p64[j]
                c = c + C[j]
            self.sum[v] = m
            self.covsum[v] = c

    def __len__(self):
        return len(self.ijk)


class MergedVoxelMap:
    """The map of the submap ids[0..m) from the parts of its keyframes: voxel v is occupied if any listed part has it; over the positions
    of `ids` whose part has v, in ascending position: S = the first part's sum, then S = S + the next one's; C likewise; n_v = sum n;
    mean_v = S / n_v, cov_v = C / n_v.  An id listed twice counts twice.  Voxels in ascending (iz, iy, ix).
    parts: the VoxelPart of every keyframe of the store (a list or a dict by id); ids: the submap."""

    def __init__(self, parts, ids):
        ids = list(ids)
        res = {parts[k].res for k in ids}
        assert len(res) == 1, "the parts of one map have one resolution"
        self.res = res.pop()
        acc = {}  # voxel -> [S, C, n], in the order of first appearance; the sums follow the order of `ids`
        for k in ids:
            p = parts[k]
            for v, key in enumerate(map(tuple, p.ijk.tolist())):
                if key not in acc:
                    acc[key] = [p.sum[v].copy(), p.covsum[v].copy(), int(p.count[v])]
                else:
                    a = acc[key]
                    a[0] = a[0] + p.sum[v]
                    a[1] = a[1] + p.covsum[v]
                    a[2] += int(p.count[v])
        keys = sorted(acc, key=lambda k: (k[2], k[1], k[0]))
        self.ijk = np.array(keys, dtype=np.int64).reshape(len(keys), 3)
        self.count = np.array([acc[k][2] for k in keys], dtype=np.int64)
        self.mean = np.array([acc[k][0] / float(acc[k][2]) for k in keys]).reshape(len(keys), 3)
        self.cov = np.array([acc[k][1] / float(acc[k][2]) for k in keys]).reshape(len(keys), 3, 3)
        self._index = {k: v for v, k in enumerate(keys)}

    def __len__(self):
        return len(self.ijk)

    def lookup(self, q_f32) -> np.ndarray:
        """voxel number of every float32 point, -1 where its voxel is empty (or out of range)."""
        ijk = voxel_of(q_f32, self.res)
        ok = np.isfinite(np.asarray(q_f32, np.float32)).all(axis=1) & (np.abs(ijk) < VOXEL_LIMIT).all(axis=1)
        return np.array([self._index.get(tuple(k), -1) if o else -1 for k, o in zip(ijk.tolist(), ok)], dtype=np.int64)


def merged_from_clouds(clouds, covs, ids, res):
    """(MergedVoxelMap, parts) of the keyframes `clouds` / `covs` (lists) for the submap `ids`; only listed keyframes get a part."""
    parts = {k: VoxelPart(clouds[k], covs[k], res) for k in sorted(set(ids))}
    return MergedVoxelMap(parts, ids), parts
