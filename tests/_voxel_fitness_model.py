"""Independent numpy (float64) model of the voxel fitness as include/ngicp.h defines it ("voxel fitness"), and the fixtures the CPU and
the GPU tests share.   *** TEST INFRASTRUCTURE ONLY ***

Built on _vgicp_model (VoxelMap, transform_f32: the float pose times the point in the passes' order), _vgicp_nbr_model.lookup_slots (the
K slots of a point) and, for the rolling case, _vgicp_rolling_model.RollingVoxelMap.  The float32 parts are spelled operation by
operation (numpy rounds every float32 operation to float32, nothing is fused); the FP64 terms are spelled in the engine's order of
operations (csrc/ngicp_math.h rotate_sym / inv3_sym, csrc/ngicp_terms.h err_term), so that the engine is expected bit-equal and held to
1e-9.  The model proves itself in test_voxel_fitness_model_cpu.py; the engine is held to it in test_gpu_voxel_fitness.py.
Not collected by pytest (no test_ prefix)."""
from __future__ import annotations

import numpy as np

import _vgicp_model as vm
import _vgicp_nbr_model as nm

DBL_MAX = float(np.finfo(np.float64).max)


# ---- the definition ------------------------------------------------------------------------------------------------------------------------
def sym6(C) -> np.ndarray:
    """(n, 3, 3) or (n, 4, 4) symmetric -> (n, 6) {xx, xy, xz, yy, yz, zz}"""
    C = np.asarray(C, np.float64)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], axis=1)


def rotate_sym6(R, A) -> np.ndarray:
    """R A R^T of n symmetric 3x3 (n, 6) in the engine's order: RA = R A row by row, each entry (r0 a0 + r1 a1) + r2 a2, then the six
    entries of the upper triangle of RA R^T the same way."""
    a00, a01, a02, a11, a12, a22 = (A[:, k] for k in range(6))
    RA = [[None] * 3 for _ in range(3)]
    for r in range(3):
        r0, r1, r2 = R[r]
        RA[r][0] = r0 * a00 + r1 * a01 + r2 * a02
        RA[r][1] = r0 * a01 + r1 * a11 + r2 * a12
        RA[r][2] = r0 * a02 + r1 * a12 + r2 * a22
    return np.stack([RA[i][0] * R[j, 0] + RA[i][1] * R[j, 1] + RA[i][2] * R[j, 2] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)


def inv3_sym6(a) -> np.ndarray:
    """the inverse of n symmetric 3x3 (n, 6) by cofactors, in the engine's order"""
    xx, xy, xz, yy, yz, zz = (a[:, k] for k in range(6))
    c00 = yy * zz - yz * yz
    c01 = xz * yz - xy * zz
    c02 = xy * yz - xz * yy
    det = xx * c00 + xy * c01 + xz * c02
    with np.errstate(all="ignore"):
        i = 1.0 / det
        return np.stack([c00 * i, c01 * i, c02 * i, (xx * zz - xz * xz) * i, (xy * xz - xx * yz) * i, (xx * yy - xy * xy) * i], axis=1)


def err_term(e, M) -> np.ndarray:
    """e^T M e of n vectors (n, 3) and matrices (n, 6), in the engine's order"""
    ex, ey, ez = e[:, 0], e[:, 1], e[:, 2]
    m00, m01, m02, m11, m12, m22 = (M[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        mex = m00 * ex + m01 * ey + m02 * ez
        mey = m01 * ex + m11 * ey + m12 * ez
        mez = m02 * ex + m12 * ey + m22 * ez
        return ex * mex + ey * mey + ez * mez


def slot_terms(src, cov_src, vmap, T, K):
    """-> (slots (n, K) voxel numbers or -1, m (n, K), d (n, K)); m and d are NaN where the slot has no voxel."""
    Tf = np.asarray(T, np.float32)
    src = np.asarray(src, np.float32)
    n = len(src)
    q = vm.transform_f32(Tf, src)
    slots = nm.lookup_slots(vmap, q, K)
    R = Tf[:3, :3].astype(np.float64)
    t = Tf[:3, 3].astype(np.float64)
    a = src.astype(np.float64)
    ta = np.stack([R[r, 0] * a[:, 0] + R[r, 1] * a[:, 1] + R[r, 2] * a[:, 2] + t[r] for r in range(3)], axis=1)  # (left to right)
    rcr = rotate_sym6(R, sym6(vm.cov3(cov_src)))
    cov_v = sym6(vmap.cov) if len(vmap) else np.zeros((0, 6))
    m = np.full((n, K), np.nan)
    d = np.full((n, K), np.nan)
    for s in range(K):
        rows = np.flatnonzero(slots[:, s] >= 0)
        if len(rows) == 0:
            continue
        v = slots[rows, s]
        e = vmap.mean[v] - ta[rows]
        M = inv3_sym6(cov_v[v] + rcr[rows])
        m[rows, s] = err_term(e, M)
        d[rows, s] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return slots, m, d


def point_values(src, cov_src, vmap, T, K):
    """-> (m (n,), d (n,), v (n,) int64, matched (n,) bool, slot_m (n, K)): a point's value is that of the winning slot - best = +inf, in
    ascending slot s wins when m_s < best; a matched point without a winner has m = d = +inf, v = -1; an unmatched one -1 / -1 / -1."""
    slots, sm, sd = slot_terms(src, cov_src, vmap, T, K)
    n = len(slots)
    matched = (slots >= 0).any(axis=1)
    best = np.full(n, np.inf)
    bd = np.full(n, np.inf)
    bv = np.full(n, -1, dtype=np.int64)
    for s in range(K):
        with np.errstate(invalid="ignore"):
            win = (slots[:, s] >= 0) & (sm[:, s] < best)  # (a NaN compares false)
        best = np.where(win, sm[:, s], best)
        bd = np.where(win, sd[:, s], bd)
        bv = np.where(win, slots[:, s], bv)
    m = np.where(matched, best, -1.0)
    d = np.where(matched, bd, -1.0)
    return m, d, bv, matched, np.where(slots >= 0, sm, np.nan)


def score(src, cov_src, vmap, T, K, max_mahalanobis=DBL_MAX) -> dict:
    """The pose's record.  The sums are plain ascending sums: the engine's fixed-order tree differs from them by rounding only."""
    m, d, _, matched, _ = point_values(src, cov_src, vmap, T, K)
    with np.errstate(invalid="ignore"):
        inl = matched & (m <= max_mahalanobis)
    k = int(inl.sum())
    return {"mahalanobis": float(m[inl].sum() / k) if k else DBL_MAX, "sqdist": float(d[inl].sum() / k) if k else DBL_MAX, "n_inliers": k, "n_matched": int(matched.sum())}


class RecordMap:
    """A voxel map given by its records (a saved rolling map: ijk, sums, covariance sums, counts), with VoxelMap's interface."""

    def __init__(self, res, ijk, sums, covsums, counts):
        self.res = res
        self.ijk = np.asarray(ijk, np.int64)
        self.count = np.asarray(counts, np.int64)
        self.mean = np.asarray(sums, np.float64) / self.count[:, None].astype(np.float64)
        self.cov = np.asarray(covsums, np.float64).reshape(-1, 3, 3) / self.count[:, None, None].astype(np.float64)
        self._index = {tuple(k): v for v, k in enumerate(self.ijk.tolist())}

    def __len__(self):
        return len(self.ijk)


# ---- the conditions under which a comparison with the engine cannot hide a failure -----------------------------------------------------------
def gate_margin(m, gates) -> float:
    """the smallest relative distance of any gate to any finite per-point m (matched points)"""
    m = np.asarray(m)
    m = m[np.isfinite(m)]  # (the caller passes the matched points' values only)
    out = np.inf
    for g in gates:
        big = np.maximum(np.abs(m), abs(g))
        rel = np.where(big > 0, np.abs(m - g) / np.where(big > 0, big, 1.0), 0.0)  # (m == g == 0: no distance at all)
        out = min(out, float(rel.min())) if len(rel) else out
    return out


def slot_gap(slot_m) -> float:
    """the smallest relative best-to-second gap among the points with two or more finite slot terms"""
    out = np.inf
    for row in np.asarray(slot_m):
        f = np.sort(row[np.isfinite(row)])
        if len(f) >= 2:
            out = min(out, float((f[1] - f[0]) / max(abs(f[1]), abs(f[0]))))
    return out


# ---- the fixtures the CPU and the GPU tests share -------------------------------------------------------------------------------------------
RES = 0.5
SIZES = (1, 63, 64, 65, 255, 256, 257, 700)
NEIGHBORS = (1, 7, 27)
GATES = (0.0, 2.5, 40.0, DBL_MAX)  # m is a squared Mahalanobis distance: chi-square-like values; 0 keeps nobody


def spd(n, seed) -> np.ndarray:
    """n random symmetric positive definite 3x3 matrices as (n, 4, 4) covariances (tests/test_gpu_vgicp_rolling.py _spd)."""
    A = np.random.default_rng(seed).normal(0, 0.1, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return out


def lattice_planes(res) -> np.ndarray:
    """Points exactly on lattice planes, negative ones included, some twice; and points just below a plane (tests/test_gpu_vgicp.py)."""
    k = np.arange(-6, 7, dtype=np.float32) * np.float32(res)
    p = np.stack(np.meshgrid(k, k[::3], k[::4], indexing="ij"), -1).reshape(-1, 3)
    below = np.nextafter(p[::5], np.float32(-np.inf))
    return np.ascontiguousarray(np.r_[p, p[::7], below, np.array([[-0.0, 0.0, -0.0]], np.float32)])


def pose(t=(0.0, 0.0, 0.0), rpy_deg=(0.0, 0.0, 0.0)) -> np.ndarray:
    """float32 4x4: Rz Ry Rx and a translation"""
    r, p, y = np.deg2rad(rpy_deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(np.float32)


POSES = {
    "identity": pose(),
    "small": pose((0.03, -0.02, 0.01), (0.4, -0.3, 0.8)),
    "several voxels": pose((1.3, -0.7, 0.4), (3.0, -2.0, 5.0)),
}


def target(seed=11):
    """(points, covariances): a random cube of half-width 2.4 plus the lattice-plane points - negative coordinates, points exactly on
    lattice planes, voxels of count 1."""
    pts = np.ascontiguousarray(np.r_[np.random.default_rng(seed).uniform(-2.4, 2.4, (900, 3)).astype(np.float32), lattice_planes(RES)])
    return pts, spd(len(pts), seed + 1)


def source(n, seed=None):
    """(points, covariances) of n source points inside the target's cube (its edge included, so that some slots leave the map)"""
    seed = 100 + n if seed is None else seed
    return np.random.default_rng(seed).uniform(-2.6, 2.6, (n, 3)).astype(np.float32), spd(n, seed + 1)


# ---- every kind of map: what the engine is driven with, and the model of the map it then holds ------------------------------------------------
KIND_RES, KIND_SRC = 1.0, 300
ROLL_POSES = (pose((0.25, -0.5, 0.125), (1.0, -2.0, 3.0)), pose((1.5, 0.75, -0.25), (-2.0, 1.0, -4.0)))
ROLL_EVICT = ((0.5, 0.0, 0.0), 4.2)  # centre, radius: voxels whose centre lies farther go


def kind_clouds():
    """two clouds with set covariances: the two keyframes of the merged map, the two scans of the rolling one; together the target"""
    a = np.random.default_rng(31).uniform(-3.0, 2.0, (500, 3)).astype(np.float32)
    b = np.random.default_rng(32).uniform(-1.0, 4.0, (400, 3)).astype(np.float32)
    return (a, spd(len(a), 33)), (b, spd(len(b), 34))


def kind_map(kind):
    """the model's map of `kind` at KIND_RES: 'target' (VoxelMap of the two clouds as one target), 'merged' (the two as keyframes of a
    submap, _vgicp_submap_model) or 'rolling' (two inserts at ROLL_POSES, then the eviction ROLL_EVICT; _vgicp_rolling_model)"""
    (a, ca), (b, cb) = kind_clouds()
    if kind == "target":
        return vm.VoxelMap(np.r_[a, b], np.r_[ca, cb], KIND_RES)
    if kind == "merged":
        import _vgicp_submap_model as sm
        return sm.MergedVoxelMap([sm.VoxelPart(a, ca, KIND_RES), sm.VoxelPart(b, cb, KIND_RES)], [0, 1])
    import _vgicp_rolling_model as rm
    m = rm.RollingVoxelMap(KIND_RES)
    m.insert(a, ca, ROLL_POSES[0])
    m.insert(b, cb, ROLL_POSES[1])
    assert m.evict(ROLL_EVICT[0], ROLL_EVICT[1], 0) > 0
    return m


def kind_source():
    return np.random.default_rng(35).uniform(-3.5, 4.5, (KIND_SRC, 3)).astype(np.float32), spd(KIND_SRC, 36)
