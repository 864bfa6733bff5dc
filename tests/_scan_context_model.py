"""The scan context definition of include/ngicp.h ("scan context") restated in numpy: float32 products and sums through explicit astype,
the ring and the sector as COUNTS, fixed-order double sums.  The tables (squared ring edges E2, boundary directions b) are inputs - the
engine's own, from scanContextTables() - and tables() below restates how the engine builds them, for the tests that need no engine.

Every function follows the header's wording line by line; nothing here is tuned to what the engine returns."""
import math

import numpy as np

F = np.float32
DEFAULTS = (20, 60, 80.0, 2.0)


def tables(R=20, S=60, L=80.0):
    """-> (E2 (R + 1,) float32, b (S / 2, 2) float32) as the header defines them"""
    L = float(F(L))
    e = np.array([F(L * k / R) for k in range(R + 1)], dtype=F)
    E2 = (e * e).astype(F)
    b = np.array([[F(math.cos(2.0 * math.pi * k / S)), F(math.sin(2.0 * math.pi * k / S))] for k in range(S // 2)], dtype=F)
    return E2, b


def cells(points, E2, b, z0=2.0):
    """-> (keep (n,) bool, ring (n,), sector (n,), v (n,) float32) of every point"""
    p = np.asarray(points, dtype=F)[:, :3]
    R, half = len(E2) - 1, len(b)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        r2 = ((x * x).astype(F) + (y * y).astype(F)).astype(F)
        keep = finite & (r2 < E2[R])
        ring = np.zeros(len(p), dtype=np.int64)
        for k in range(1, R):
            ring += r2 >= E2[k]
        low = (y < 0) | ((y == 0) & (x < 0))
        xs, ys = np.where(low, -x, x).astype(F), np.where(low, -y, y).astype(F)
        sector = np.where(low, half, 0).astype(np.int64)
        for k in range(1, half):
            cross = ((b[k, 0] * ys).astype(F) - (b[k, 1] * xs).astype(F)).astype(F)
            sector += cross >= 0
        v = (z + F(z0)).astype(F)
    return keep, ring, sector, v


def descriptor(points, E2, b, z0=2.0):
    """-> D (R, S) float32"""
    R, S = len(E2) - 1, 2 * len(b)
    D = np.zeros((R, S), dtype=F)
    if len(points) == 0:
        return D
    keep, ring, sector, v = cells(points, E2, b, z0)
    np.maximum.at(D, (ring[keep], sector[keep]), v[keep])  # (cells start at 0.0f, so a v <= 0 leaves them there)
    return D


def norms(D):
    """column norms, summed in double with r ascending from 0.0"""
    D = np.asarray(D, dtype=F).astype(np.float64)
    s = np.zeros(D.shape[1])
    for r in range(D.shape[0]):
        s = s + D[r] * D[r]
    return np.sqrt(s)


def shift_distances(Q, C):
    """-> d (S,) float64: d_k for every shift k"""
    Q64, C64 = np.asarray(Q, dtype=F).astype(np.float64), np.asarray(C, dtype=F).astype(np.float64)
    R, S = Q64.shape
    nq, nc = norms(Q), norms(C)
    d = np.empty(S)
    for k in range(S):
        jp = (np.arange(S) + k) % S
        Ck, nck = C64[:, jp], nc[jp]
        dot = np.zeros(S)
        for r in range(R):
            dot = dot + Q64[r] * Ck[r]
        counted = (nq > 0) & (nck > 0)
        total, m = 0.0, 0
        for j in np.flatnonzero(counted):  # j ascending
            total = total + dot[j] / (nq[j] * nck[j])
            m += 1
        d[k] = 1.0 - total / float(m) if m else 1.0
    return d


def distance(Q, C):
    """-> (dist, shift): the minimum over the shifts and the smallest k that attains it (k ascending under strict <)"""
    d = shift_distances(Q, C)
    best, shift = d[0], 0
    for k in range(1, len(d)):
        if d[k] < best:
            best, shift = d[k], k
    return float(best), shift


def distances(Q, database):
    r = [distance(Q, C) for C in database]
    return np.array([x[0] for x in r], dtype=np.float64), np.array([x[1] for x in r], dtype=np.int32)


def ranking(dist, first=0):
    """ids ascending by (distance, id)"""
    dist = np.asarray(dist)
    ids = np.arange(len(dist)) + first
    return ids[np.lexsort((ids, dist))]


def match(Q, database, begin, end, top_k):
    """-> (ids, dist, shift) of the first min(top_k, end - begin) entries of the ranking of database[begin:end]"""
    dist, shift = distances(Q, database[begin:end])
    order = ranking(dist)[:top_k]
    return (order + begin).astype(np.int32), dist[order], shift[order]


def guess(shift, S=60):
    """the rotation about z by shift * 2 pi / S, float32 4x4"""
    a = float(shift) * (2.0 * np.pi / S)
    T = np.eye(4, dtype=F)
    T[0, 0] = T[1, 1] = F(np.cos(a))
    T[1, 0] = F(np.sin(a))
    T[0, 1] = -T[1, 0]
    return T


def cell_centre_cloud(E2, b, heights):
    """one point per cell with heights[ring, sector] > 0, at the cell's centre (mid radius, mid angle), z = height - 2 (z0 = 2):
    well inside the cell, so a rotation by whole sectors moves every point to the centre of another cell"""
    R, S = heights.shape
    e = np.sqrt(np.asarray(E2, dtype=np.float64))
    pts = []
    for r in range(R):
        for s in range(S):
            if heights[r, s] > 0:
                rad, ang = 0.5 * (e[r] + e[r + 1]), (s + 0.5) * 2.0 * np.pi / S
                pts.append((rad * np.cos(ang), rad * np.sin(ang), float(heights[r, s]) - 2.0))
    return np.array(pts, dtype=F).reshape(-1, 3)


def rotate_z(points, angle):
    c, s = np.cos(angle), np.sin(angle)
    p = np.asarray(points, dtype=np.float64)
    return np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1], p[:, 2]], axis=1).astype(F)
