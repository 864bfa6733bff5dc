"""Independent numpy (float64) model of the rolling map's clearing along rays as include/ngicp.h defines it ("rolling voxel map: clearing
along rays").   *** TEST INFRASTRUCTURE ONLY ***

Vectorised over the rays with a loop over the steps.  Every expression of the definition is spelled operation by operation: numpy rounds
each operation to its type and fuses nothing.  Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

from _vgicp_model import VOXEL_LIMIT, voxel_of
from _vgicp_rolling_model import transform_pcl_f32

DEFAULTS = dict(near_cells=1, back_cells=2, max_steps=4096, min_miss=2, radius_cells=0.25, keep_stamp=0, dry_run=0)
BIAS = 1 << 20


class Refused(ValueError):
    """the origin or a transformed point has no cell"""


def cells_of(p, res):
    """-> (ijk (n, 3) int64, ok (n,)): the cell of every float32 point by the mode's rule, ok False where it has none"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    ijk = voxel_of(p, res)
    return ijk, np.isfinite(p).all(axis=1) & (np.abs(ijk) < VOXEL_LIMIT).all(axis=1)


def pack(ijk):
    ijk = np.asarray(ijk, np.int64)
    return ((ijk[..., 2] + BIAS) << 42) | ((ijk[..., 1] + BIAS) << 21) | (ijk[..., 0] + BIAS)


class Rays:
    """What the walk starts from: od, d, c0, c1, n_a, s_a, inv_a and N per ray."""

    def __init__(self, origin, q, res):
        o = np.asarray(origin, np.float32).reshape(3)
        q = np.asarray(q, np.float32).reshape(-1, 3)
        c0, ok0 = cells_of(o, res)
        c1, ok1 = cells_of(q, res)
        if not ok0.all() or not ok1.all():
            raise Refused("the origin or a point has no cell")
        self.res = np.float64(res)
        self.od = o.astype(np.float64)
        self.d = q.astype(np.float64) - self.od
        self.c0, self.c1 = c0[0], c1
        dc = c1 - c0[0]
        self.n = np.abs(dc)
        self.s = np.sign(dc)
        self.N = self.n.sum(axis=1)
        with np.errstate(divide="ignore"):
            self.inv = 1.0 / self.d  # (read only where n_a > 0)

    def steps(self, last):
        """The walk: yields (j, idx, cells) for j = 1, 2, ... - the rays idx with last[idx] >= j, and the cell each is in behind step j."""
        last = np.asarray(last, np.int64)
        cur = np.tile(self.c0, (len(self.N), 1))
        k = np.zeros_like(cur)
        up = (self.s > 0).astype(np.int64)
        for j in range(1, int(last.max(initial=0)) + 1):
            idx = np.flatnonzero(last >= j)
            cand = k[idx] < self.n[idx]
            assert cand.any(axis=1).all()  # (last <= N: a step is left)
            with np.errstate(invalid="ignore", over="ignore"):
                t = ((cur[idx] + up[idx]).astype(np.float64) * self.res - self.od) * self.inv[idx]
            t = np.where(cand, t, np.inf)
            ax = np.argmin(t, axis=1)  # (the first of equal minima: x before y before z)
            cur[idx, ax] += self.s[idx, ax]
            k[idx, ax] += 1
            yield j, idx, cur[idx].copy()

    def full_walk(self):
        """-> cells (n, max N + 1, 3) with row [i, j] the cell of ray i behind step j (j = 0: c0; rows past N_i repeat the last cell)"""
        n, top = len(self.N), int(self.N.max(initial=0))
        out = np.empty((n, top + 1, 3), np.int64)
        out[:, 0] = self.c0
        for j, idx, cells in self.steps(self.N):
            out[:, j] = out[:, j - 1]
            out[idx, j] = cells
        return out


def ray_counts(ijk, mean, res, q, origin, near_cells=1, back_cells=2, max_steps=4096, radius_cells=0.25, **_):
    """miss, hit (V,) uint32 and the totals {steps, occupied, misses} of the rays origin -> q (float32, already in the map frame) against
    the map with the cells ijk (V, 3) and the record means mean (V, 3)."""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    mean = np.asarray(mean, np.float64).reshape(-1, 3)
    V = len(ijk)
    rays = Rays(origin, q, res)
    keys = pack(ijk)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]

    def lookup(cells):
        if V == 0:
            return np.full(len(cells), -1, np.int64)
        kk = pack(cells)
        pos = np.minimum(np.searchsorted(skeys, kk), V - 1)
        return np.where(skeys[pos] == kk, order[pos], -1)

    miss, hit = np.zeros(V, np.int64), np.zeros(V, np.int64)
    steps = occupied = misses = 0
    r = np.float64(radius_cells) * np.float64(res)
    r2 = r * r
    d = rays.d
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    last = np.minimum(rays.N - 1 - int(back_cells), int(max_steps))
    for j, idx, cells in rays.steps(last):
        if j < near_cells:
            continue
        steps += len(idx)
        v = lookup(cells)
        occ = v >= 0
        occupied += int(occ.sum())
        i, v = idx[occ], v[occ]
        if radius_cells > 0:
            w = mean[v] - rays.od
            di = d[i]
            ts = ((w[:, 0] * di[:, 0] + w[:, 1] * di[:, 1]) + w[:, 2] * di[:, 2]) / dd[i]
            e = w - ts[:, None] * di
            v = v[((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) <= r2]
        misses += len(v)
        np.add.at(miss, v, 1)
    v = lookup(rays.c1)
    np.add.at(hit, v[v >= 0], 1)
    return dict(miss=miss.astype(np.uint32), hit=hit.astype(np.uint32), steps=steps, occupied=occupied, misses=misses)


def ray_clear(ijk, mean, stamp, res, points, T, origin=None, **options):
    """The whole entry on a map given by its arrays: the counts of ray_counts for the producer's points at the float pose T, and
    keep (V,) bool - the voxels that stay - with n_removed.  (A dry run removes nothing: keep is all True.)"""
    o = {**DEFAULTS, **options}
    Tf = np.asarray(T, np.float32)
    q = transform_pcl_f32(Tf, points)
    org = Tf[:3, 3] if origin is None else np.asarray(origin, np.float32)
    out = ray_counts(ijk, mean, res, q, org, **o)
    stamp = np.asarray(stamp, np.int64)
    gone = (out["miss"] >= o["min_miss"]) & (out["hit"] == 0) & ((o["keep_stamp"] <= 0) | (stamp < o["keep_stamp"]))
    if o["dry_run"]:
        gone = np.zeros_like(gone)
    out["keep"] = ~gone
    out["n_removed"] = int(gone.sum())
    return out
