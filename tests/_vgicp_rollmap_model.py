"""Independent numpy (float64) model of the rolling voxel map's record routes as include/ngicp.h defines them ("rolling voxel map:
records"): restore, insert of records at a pose, move in place.   *** TEST INFRASTRUCTURE ONLY ***

RecordVoxelMap is _vgicp_rolling_model.RollingVoxelMap (scan inserts, eviction, the vmap interface of the pass models) with the three
record entries on top; it reuses that model's rotate_sym, transform_pcl_f32 and voxel_of.  Every sum is taken term by term in the
stated order, and numpy rounds every operation to its type: nothing is fused.  Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

from _vgicp_model import VOXEL_LIMIT, voxel_of
from _vgicp_rolling_model import Refused, RollingVoxelMap, rotate_sym, transform_pcl_f32

COUNT_MAX = 2 ** 31 - 1


def sym3(C) -> np.ndarray:
    """(n, 6) {xx, xy, xz, yy, yz, zz} or (n, 3, 3) -> (n, 3, 3) float64"""
    c = np.asarray(C, np.float64)
    return c if c.ndim == 3 else c.reshape(-1, 6)[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


class RecordVoxelMap(RollingVoxelMap):
    # ---- restore ----
    def set(self, ijk, S, C, count, stamp, inserts):
        """The map becomes exactly the given state; raises Refused (and changes nothing) on what the header lists."""
        ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
        S, C = np.asarray(S, np.float64).reshape(-1, 3), sym3(C)
        count, stamp = np.asarray(count, np.int64).reshape(-1), np.asarray(stamp, np.int64).reshape(-1)
        if inserts < 0:
            raise Refused("a negative insert counter")
        if (np.abs(ijk) >= VOXEL_LIMIT).any() or (count < 1).any() or (count > COUNT_MAX).any() or (stamp < 1).any() or (stamp > inserts).any():
            raise Refused("an index, count or stamp out of range")
        keys = list(map(tuple, ijk.tolist()))
        seen = {}
        for v, k in enumerate(keys):
            if k in seen:
                raise Refused(f"rows {seen[k]} and {v} name the same voxel")
            seen[k] = v
        self._acc = {k: [S[v].copy(), C[v].copy(), int(count[v]), int(stamp[v])] for v, k in enumerate(keys)}
        self._order = keys
        self.inserts = int(inserts)
        self._refresh()

    # ---- the definition of an insert of records ----
    def record_sums(self, S, C, count, T, stamps=None):
        """Per destination voxel {key: (s, c, N, largest stamp)} and the keys in ascending (iz, iy, ix).  Raises Refused for a count
        below 1 or a moved mean without a voxel."""
        S, C = np.asarray(S, np.float64).reshape(-1, 3), sym3(C)
        count = np.asarray(count, np.int64).reshape(-1)
        if len(count) == 0:
            raise Refused("no records")
        if (count < 1).any():
            raise Refused("a count below 1")
        Tf = np.asarray(T, np.float32)
        with np.errstate(all="ignore"):
            m = S / count.astype(np.float64)[:, None]  # three divisions per record
            p = m.astype(np.float32)
        q = transform_pcl_f32(Tf, p)
        ijk = voxel_of(q, self.res)
        if not np.isfinite(q).all() or (np.abs(ijk) >= VOXEL_LIMIT).any():
            raise Refused("a record's moved mean lies 2^20 voxels or more from the origin (or is not finite)")
        R = Tf[:3, :3].astype(np.float64)
        t = Tf[:3, 3].astype(np.float64)
        groups = {}
        for r, key in enumerate(map(tuple, ijk.tolist())):  # ascending input index
            groups.setdefault(key, []).append(r)
        out = {}
        for key, idx in groups.items():
            A, Cc, N, newest = np.zeros(3), np.zeros((3, 3)), 0, 0
            for r in idx:  # one after the other: the order of the sum is part of the definition
                A = A + S[r]
                Cc = Cc + C[r]
                N += int(count[r])
                if stamps is not None:
                    newest = max(newest, int(stamps[r]))
            s = np.array([((R[k, 0] * A[0] + R[k, 1] * A[1]) + R[k, 2] * A[2]) + np.float64(N) * t[k] for k in range(3)])
            out[key] = (s, rotate_sym(R, Cc), N, newest)  # ONE rotation per destination voxel
        return out, sorted(out, key=lambda k: (k[2], k[1], k[0]))

    def insert_records(self, S, C, count, T):
        """-> (voxels created, destination voxels).  A refused insert raises before anything is written."""
        sums, keys = self.record_sums(S, C, count, T)
        for key in keys:
            if sums[key][2] + (self._acc[key][2] if key in self._acc else 0) > COUNT_MAX:
                raise Refused("a voxel's count would pass 2^31 - 1")
        stamp = self.inserts + 1
        n_new = 0
        for key in keys:  # new voxels are numbered in ascending (iz, iy, ix)
            s, c, N, _ = sums[key]
            if key in self._acc:
                a = self._acc[key]
                a[0] = a[0] + s
                a[1] = a[1] + c
                a[2] += N
                a[3] = stamp
            else:
                self._acc[key] = [s.copy(), c.copy(), N, stamp]
                self._order.append(key)
                n_new += 1
        self.inserts = stamp
        self._refresh()
        return n_new, len(keys)

    def insert_map(self, other, T):
        return self.insert_records(other.sum, other.covsum, other.count, T)

    # ---- move in place ----
    def transform(self, T):
        """-> voxels after the move.  The former records, in their former numbering, inserted into an empty map; the counter stays; a
        destination voxel carries the largest stamp of its records."""
        if not self._order:
            return 0
        sums, keys = self.record_sums(self.sum, self.covsum, self.count, T, self.stamp)
        for key in keys:
            if sums[key][2] > COUNT_MAX:
                raise Refused("a voxel's count would pass 2^31 - 1")
        self._acc = {key: [sums[key][0].copy(), sums[key][1].copy(), sums[key][2], sums[key][3]] for key in keys}
        self._order = list(keys)
        self._refresh()
        return len(keys)

    def records(self):
        """(ijk, S, C (n, 3, 3), count, stamp): what rollingVoxelMap() returns"""
        return self.ijk.copy(), self.sum.copy(), self.covsum.copy(), self.count.copy(), self.stamp.copy()
