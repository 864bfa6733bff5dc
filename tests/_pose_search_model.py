"""Independent numpy model of the voxel pose search as include/ngicp.h defines it ("voxel pose search").   *** TEST INFRASTRUCTURE ONLY ***

The score is an integer, so the engine is held to this model with np.array_equal.  The float32 parts - the float pose times the point,
the cell of the result - are _vgicp_model's transform_f32 and voxel_of.  score_volume is vectorised (a dense occupancy array where the
map's box is small, sorted packed keys where it is not); naive_volume is the definition spelled as a loop over points and shifts, and
tests/test_pose_search_model_cpu.py holds the one to the other.  Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

from _vgicp_model import VOXEL_LIMIT, transform_f32, voxel_of

MAX_EXTENT_XY, MAX_EXTENT_Z, MAX_SHIFTS, MAX_ENTRIES, MAX_TOP_K = 31, 7, 12288, 1 << 24, 64
MAX_GRID_BYTES = 256 << 20
DENSE_CELLS = 1 << 24  # the dense route's cap; beyond it the sparse one


def cells(T, src, res):
    """-> (ijk (n, 3) int64, has (n,) bool): c_b(p) of every source point at the float pose T and whether the point has a cell"""
    with np.errstate(all="ignore"):
        q = transform_f32(np.asarray(T, np.float32), src)
        ijk = voxel_of(q, res)
    has = np.isfinite(q).all(axis=1) & (np.abs(ijk) < VOXEL_LIMIT).all(axis=1)
    return ijk, has


def shifts(extent) -> np.ndarray:
    """(|S|, 3) int64 in index order: sx fastest, sz slowest"""
    ex, ey, ez = extent
    sz, sy, sx = np.meshgrid(np.arange(-ez, ez + 1), np.arange(-ey, ey + 1), np.arange(-ex, ex + 1), indexing="ij")
    return np.stack([sx.ravel(), sy.ravel(), sz.ravel()], axis=1).astype(np.int64)


def shift_index(s, extent) -> int:
    ex, ey, ez = extent
    return ((s[2] + ez) * (2 * ey + 1) + (s[1] + ey)) * (2 * ex + 1) + (s[0] + ex)


def _pack(ijk):
    k = np.asarray(ijk, np.int64) + VOXEL_LIMIT
    return (k[..., 2] << 42) | (k[..., 1] << 21) | k[..., 0]


def naive_volume(Ts, src, map_ijk, res, extent) -> np.ndarray:
    """the definition, one point and one shift at a time"""
    ex, ey, ez = extent
    occupied = {tuple(int(v) for v in k) for k in np.asarray(map_ijk).reshape(-1, 3)}
    out = np.zeros((len(Ts), 2 * ez + 1, 2 * ey + 1, 2 * ex + 1), dtype=np.int32)
    for b, T in enumerate(Ts):
        ijk, has = cells(T, src, res)
        for c, h in zip(ijk.tolist(), has):
            if not h:
                continue
            for sz in range(-ez, ez + 1):
                for sy in range(-ey, ey + 1):
                    for sx in range(-ex, ex + 1):
                        v = (c[0] + sx, c[1] + sy, c[2] + sz)
                        if all(-VOXEL_LIMIT < a < VOXEL_LIMIT for a in v) and v in occupied:
                            out[b, sz + ez, sy + ey, sx + ex] += 1
    return out


def score_volume(Ts, src, map_ijk, res, extent, force_sparse=False) -> np.ndarray:
    """(B, 2 ez + 1, 2 ey + 1, 2 ex + 1) int32.  A map cell is always in range, so `c + s in the map` implies the range rule."""
    ex, ey, ez = extent
    S = shifts(extent)
    m = np.unique(np.asarray(map_ijk, np.int64).reshape(-1, 3), axis=0)
    out = np.zeros((len(Ts), len(S)), dtype=np.int32)
    if len(m) == 0:
        return out.reshape(len(Ts), 2 * ez + 1, 2 * ey + 1, 2 * ex + 1)
    e = np.array(extent, np.int64)
    near_lo, near_hi = m.min(axis=0) - e, m.max(axis=0) + e  # a source cell outside this box has no map cell in its window
    lo = near_lo - e                                          # the dense array: the window of every such cell lies inside it
    dims = near_hi + e - lo + 1
    dense = not force_sparse and int(np.prod(dims.astype(object))) <= DENSE_CELLS
    if dense:
        occ = np.zeros(tuple(dims), dtype=bool)
        occ[tuple((m - lo).T)] = True
        occ = occ.ravel()
        stride = np.array([dims[1] * dims[2], dims[2], 1], np.int64)
        off = S @ stride
    else:
        keys = np.sort(_pack(m))
    for b, T in enumerate(Ts):
        ijk, has = cells(T, src, res)
        u, w = np.unique(ijk[has], axis=0, return_counts=True)  # duplicates count each time
        near = ((u >= near_lo) & (u <= near_hi)).all(axis=1)
        u, w = u[near], w[near]
        if len(u) == 0:
            continue
        if dense:
            base = (u - lo) @ stride
        for at in range(0, len(S), 2048):  # (bounded temporaries)
            if dense:
                hit = occ[base[:, None] + off[None, at:at + 2048]]
            else:
                v = u[:, None, :] + S[None, at:at + 2048, :]
                ok = (np.abs(v) < VOXEL_LIMIT).all(axis=-1)
                k = _pack(np.where(ok[..., None], v, 0))
                pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
                hit = ok & (keys[pos] == k)
            out[b, at:at + 2048] = w @ hit.astype(np.int64)
    return out.reshape(len(Ts), 2 * ez + 1, 2 * ey + 1, 2 * ex + 1)


def ranking(volume, top_k):
    """-> (pose, shift (m, 3), score): the first min(top_k, B |S|) entries by descending score, ascending pose, ascending shift index"""
    B, wz, wy, wx = volume.shape
    flat = volume.reshape(-1).astype(np.int64)
    order = np.lexsort((np.arange(len(flat)), -flat))[:top_k]
    per = wz * wy * wx
    pose, idx = order // per, order % per
    shift = np.stack([idx % wx - (wx - 1) // 2, (idx // wx) % wy - (wy - 1) // 2, idx // (wx * wy) - (wz - 1) // 2], axis=1)
    return pose.astype(np.int32), shift.astype(np.int32), flat[order].astype(np.int32)


def candidate_pose(T, shift, res) -> np.ndarray:
    """T with its translation replaced, per axis, by (float)((double)t + (double)s * res)"""
    out = np.array(T, dtype=np.float32)
    for a in range(3):
        out[a, 3] = np.float32(np.float64(out[a, 3]) + np.float64(int(shift[a])) * np.float64(res))
    return out


def yaw_lattice(T0, n, step_rad) -> np.ndarray:
    """T0 . Rz(k step) as float32 (the engine's helper returns the same poses; both sides take them as input)"""
    out = np.empty((n, 4, 4), dtype=np.float32)
    for k in range(n):
        a = k * float(step_rad)
        Rz = np.eye(4)
        Rz[0, 0] = Rz[1, 1] = np.cos(a)
        Rz[1, 0] = np.sin(a)
        Rz[0, 1] = -Rz[1, 0]
        out[k] = (np.asarray(T0, np.float64) @ Rz).astype(np.float32)
    return out


# ---- the boxes and the grid plan (csrc/ngicp_pose_search_plan.h restated) ----
EMPTY_BOX = (np.array([2**31 - 1] * 3, dtype=np.int64), np.array([-2**31] * 3, dtype=np.int64))


def box_of(ijk):
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    return (ijk.min(axis=0), ijk.max(axis=0)) if len(ijk) else EMPTY_BOX


def source_box(Ts, src, res):
    got = [ijk[has] for ijk, has in (cells(T, src, res) for T in Ts)]
    return box_of(np.concatenate(got) if got else np.zeros((0, 3)))


def plan(map_box, src_box, extent):
    """-> None for an empty intersection, else dict(org, n, row_words, bytes, too_large)"""
    e = np.asarray(extent, np.int64)
    if (map_box[0] > map_box[1]).any() or (src_box[0] > src_box[1]).any():
        return None
    lo, hi = np.maximum(map_box[0], src_box[0] - e), np.minimum(map_box[1], src_box[1] + e)
    if (lo > hi).any():
        return None
    n = hi - lo + 1
    row_words = (int(n[0]) + 63) // 64 + 2
    nbytes = row_words * int(n[1]) * int(n[2]) * 8
    return dict(org=lo, n=n, row_words=row_words, bytes=nbytes, too_large=nbytes > MAX_GRID_BYTES)
