"""Independent numpy model of moving keyframes as include/ngicp.h defines it ("moving keyframes").   *** TEST INFRASTRUCTURE ONLY ***

A store is a list of (points (n, 3) float32, covs (n, 4, 4) float64) in original point order.  move() applies, per listed keyframe,
the float32 transform of _vgicp_rolling_model.transform_pcl_f32 to the points and ONE _vgicp_rolling_model.rotate_sym per point to the
covariances (R the float 3x3 block widened to double) - the covariances are not recomputed - and refuses what the header refuses,
changing nothing.  numpy rounds every operation to its type; nothing is fused.  Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

from _vgicp_rolling_model import rotate_sym, transform_pcl_f32


class Refused(ValueError):
    """a call the header answers with NGICP_ERR_ARG; the store is as it was"""


def move_one(points, covs, T):
    """-> (points', covs') of one keyframe under the float matrix T (4, 4, row-major as numpy holds it)."""
    Tf = np.asarray(T, np.float32)
    p = np.asarray(points, np.float32)
    q = transform_pcl_f32(Tf, p)
    R = Tf[:3, :3].astype(np.float64)
    c = np.asarray(covs, np.float64)
    out = np.zeros_like(c)
    for i in range(len(c)):
        out[i, :3, :3] = rotate_sym(R, c[i, :3, :3])
    return q, out


def check_args(n_keyframes, ids, Ts):
    if ids is None or Ts is None or len(ids) == 0:
        raise Refused("null ids or transforms, or an empty list")
    ids = [int(i) for i in ids]
    Ts = np.asarray(Ts, np.float32)
    if Ts.shape != (len(ids), 4, 4):
        raise Refused("one 4x4 per id")
    for i in ids:
        if i < 0 or i >= n_keyframes:
            raise Refused(f"unknown keyframe id {i}")
    first = {}
    for pos, i in enumerate(ids):
        if i in first:
            raise Refused(f"keyframe {i} is listed twice, at positions {first[i]} and {pos}")
        first[i] = pos
    for j, T in enumerate(Ts):
        if not np.isfinite(T).all():
            raise Refused(f"transform {j} has an entry that is not finite")
        if not np.array_equal(T[3], np.array([0, 0, 0, 1], np.float32)):
            raise Refused(f"the last row of transform {j} is not (0, 0, 0, 1)")
    return ids, Ts


def move(store, ids, Ts):
    """-> the store after ngicp_keyframe_transform(ids, Ts): a new list; `store` itself is never written.  Raises Refused."""
    ids, Ts = check_args(len(store), ids, Ts)
    moved = {}
    for i, T in zip(ids, Ts):
        q, c = move_one(store[i][0], store[i][1], T)
        if not np.isfinite(q).all():
            raise Refused("a moved coordinate is not finite")
        moved[i] = (q, c)
    return [moved.get(i, kf) for i, kf in enumerate(store)]


def box(points):
    p = np.asarray(points, np.float32)
    return p.min(axis=0), p.max(axis=0)
