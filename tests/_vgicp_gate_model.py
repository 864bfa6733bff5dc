"""Independent numpy (float64) model of the gated insert as include/ngicp.h defines it ("rolling voxel map: gated insert"), and the
fixtures the CPU and the GPU tests share.   *** TEST INFRASTRUCTURE ONLY ***

classify() is _voxel_fitness_model.slot_terms (the per-slot terms of voxel fitness) with the count mask and the winner rule; gated_insert()
is _vgicp_rolling_model.RollingVoxelMap.insert of the kept rows.  Not collected by pytest (no test_ prefix)."""
from __future__ import annotations

import functools

import numpy as np

import _vgicp_model as vm
import _vgicp_rolling_model as rm
import _voxel_fitness_model as fm

DBL_MAX = fm.DBL_MAX
NEW, EXPLAINED, CONFLICT, UNJUDGED = 0, 1, 2, 3
DEFAULTS = dict(min_voxel_count=1, insert_new=1, insert_unjudged=1, dry_run=0)


# ---- the definition ------------------------------------------------------------------------------------------------------------------------
def classify(src, cov_src, vmap, T, K, max_mahalanobis, min_voxel_count=1):
    """-> (cls (n,) uint8, best (n,) the winner's m or +inf, slot_m (n, K): the judging slots' terms, NaN elsewhere)"""
    slots, m, _ = fm.slot_terms(src, cov_src, vmap, T, K)
    n = len(slots)
    occ = slots >= 0
    count = np.asarray(vmap.count, np.int64) if len(vmap) else np.zeros(0, np.int64)
    judge = occ & ((count[np.where(occ, slots, 0)] if len(count) else np.zeros_like(slots)) >= min_voxel_count)
    best = np.full(n, np.inf)
    won = np.zeros(n, bool)
    for s in range(K):  # ascending slot: a tie stays with the lower one; NaN and +inf compare false
        with np.errstate(invalid="ignore"):
            w = judge[:, s] & (m[:, s] < best)
        best = np.where(w, m[:, s], best)
        won |= w
    with np.errstate(invalid="ignore"):
        cls = np.where(~occ.any(axis=1), NEW, np.where(~won, UNJUDGED, np.where(best <= max_mahalanobis, EXPLAINED, CONFLICT)))
    return cls.astype(np.uint8), best, np.where(judge, m, np.nan)


def kept(cls, insert_new=1, insert_unjudged=1):
    return (cls == EXPLAINED) | ((cls == NEW) & bool(insert_new)) | ((cls == UNJUDGED) & bool(insert_unjudged))


def gated_insert(m: rm.RollingVoxelMap, src, cov_src, T, K, max_mahalanobis, **options):
    """The whole entry on the model's map `m` -> {cls, n_points, n_class, n_kept, n_new, n_touched; best, slot_m as classify gives them}.  The refusal is the plain insert's,
    judged on every point before anything is written (raises rm.Refused); nothing kept, or a dry run, leaves the map and its counter."""
    unknown = set(options) - set(DEFAULTS)
    assert not unknown, unknown
    o = {**DEFAULTS, **options}
    src = np.asarray(src, np.float32)
    q = rm.transform_pcl_f32(T, src)  # the INSERT's transform, not the gate's
    if not np.isfinite(q).all() or (np.abs(vm.voxel_of(q, m.res)) >= vm.VOXEL_LIMIT).any():
        raise rm.Refused("a transformed point lies 2^20 voxels or more from the origin (or is not finite)")
    cls, best, slot_m = classify(src, cov_src, m, T, K, max_mahalanobis, o["min_voxel_count"])
    keep = kept(cls, o["insert_new"], o["insert_unjudged"])
    n_new = n_touched = 0
    if keep.any() and not o["dry_run"]:
        n_new, n_touched = m.insert(src[keep], np.asarray(cov_src)[keep], T)
    return dict(cls=cls, n_points=len(src), n_class=[int((cls == k).sum()) for k in range(4)], n_kept=int(keep.sum()), n_new=n_new, n_touched=n_touched,
                best=best, slot_m=slot_m)


def classes_from_point_values(m, v, max_mahalanobis):
    """the classes under min_voxel_count == 1 from voxel_fitness_points' m and v: v = -1 and m = -1 is NEW, m = +inf is UNJUDGED"""
    m, v = np.asarray(m), np.asarray(v)
    with np.errstate(invalid="ignore"):
        return np.where((v == -1) & (m == -1.0), NEW, np.where(np.isposinf(m), UNJUDGED, np.where(m <= max_mahalanobis, EXPLAINED, CONFLICT))).astype(np.uint8)


# ---- the fixtures the CPU and the GPU tests share -------------------------------------------------------------------------------------------
RES = fm.RES  # 0.5
SIZES = fm.SIZES + (4097,)  # (one past a scan tile, kScanTile = 4096 in csrc/ngicp_grid.h: the keep flags' scan then takes two tiles)
NEIGHBORS = fm.NEIGHBORS
GATES = fm.GATES
FLOOR = 5e-2  # the smallest share of a class in the fixture source (K = 7, FIX_GATE, FIX_MIN_COUNT)
FIX_GATE, FIX_MIN_COUNT = 2.5, 3
MARGIN = 1e-6  # the floors of tests/test_voxel_fitness_model_cpu.py: no m within 1e-6 (relative) of a gate or of its runner-up
MAP_POSES = (fm.pose(), fm.pose((0.03, -0.02, 0.01), (0.4, -0.3, 0.8)), fm.pose((-0.02, 0.04, 0.0), (0.0, 0.5, -0.6)))
SRC_POSE = fm.pose((0.02, 0.01, -0.005), (0.2, -0.1, 0.3))


def covs(n, seed) -> np.ndarray:
    """n covariances (n, 4, 4) of points on a horizontal surface: loose along it, tight across it, each a little different"""
    A = np.random.default_rng(seed).normal(0, 0.004, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + np.diag([0.04, 0.04, 0.0004])
    return out


def _floor(n, seed, x, y, z=0.1):
    r = np.random.default_rng(seed)
    return np.stack([r.uniform(*x, n), r.uniform(*y, n), z + r.normal(0, 0.004, n)], axis=1).astype(np.float32)


def map_scans():
    """the three scans that build the fixture map: a dense floor with the lattice-plane points (cells' edges, -0.0), the floor's left
    half again (counts differ), and a sparse strip of one or two points per voxel"""
    a = np.ascontiguousarray(np.r_[_floor(1500, 1, (-3, 3), (-3, 3)), fm.lattice_planes(RES)])
    b = _floor(500, 2, (-3, 0), (-3, 3))
    c = _floor(70, 3, (3.25, 5.75), (-3, 3))
    return [(a, covs(len(a), 11), MAP_POSES[0]), (b, covs(len(b), 12), MAP_POSES[1]), (c, covs(len(c), 13), MAP_POSES[2])]


def build_map(n_scans=3) -> rm.RollingVoxelMap:
    m = rm.RollingVoxelMap(RES)
    for pts, cv, T in map_scans()[:n_scans]:
        m.insert(pts, cv, T)
    return m


@functools.lru_cache(maxsize=None)
def source(n, seed=None):
    """(points, covariances) of n source points, by index modulo 8: on the dense floor (0, 1, 2), a slab lifted 0.12 .. 0.3 m off it
    (3, 4: CONFLICT), beyond the map (5: NEW), on the sparse strip (6, 7: UNJUDGED under min_voxel_count = 3, or NEW)"""
    seed = 500 + n if seed is None else seed
    r = np.random.default_rng(seed)
    kind = np.arange(n) % 8
    p = np.empty((n, 3))
    p[:, 0] = r.uniform(-2.7, 2.7, n)
    p[:, 1] = r.uniform(-2.7, 2.7, n)
    p[:, 2] = 0.1 + r.normal(0, 0.004, n)
    lifted = (kind == 3) | (kind == 4)
    p[lifted, 2] += r.uniform(0.12, 0.3, int(lifted.sum()))
    p[kind == 5, 0] -= 6.5
    strip = kind >= 6
    p[strip, 0] = r.uniform(3.3, 5.7, int(strip.sum()))
    return np.ascontiguousarray(p, dtype=np.float32), covs(n, seed + 1)


# several gated inserts in a row, from an empty map on: (points, pose, gate, options); the third keeps nothing
RUN = (
    (700, MAP_POSES[0], 2.5, {}),
    (257, MAP_POSES[1], 2.5, dict(min_voxel_count=3)),
    (65, SRC_POSE, 0.0, dict(insert_new=0, insert_unjudged=0)),
    (1030, MAP_POSES[2], 40.0, dict(insert_unjudged=0)),
    (255, SRC_POSE, 2.5, dict(min_voxel_count=3, insert_new=0)),
)


# ---- the drive: tests/_vgicp_ray_drive.py's room with the moving box, inserted frame by frame at the true pose --------------------------------
DRIVE_RES, DRIVE_K, DRIVE_STRIDE = 1.0, 7, 2  # (every second ray: the covariances below cost n^2)
DRIVE_FRAMES = 7                              # frames 0 .. 6: what _vgicp_ray_drive.trail_mask labels
# Chosen on the model (test_vgicp_gate_model_cpu.py pins them): the covariances are plane-regularised - 1 along a surface, 1e-3 across it -
# so m sees only the offset across a surface and a chi-square-sized gate (7.8) keeps the whole scan; 0.5 is where the box's sides start to
# be told from the floor beside them.  The first frame founds the map ungated.  Figures: (trail voxels ungated, gated, static lost, static).
DRIVE_GATE, DRIVE_MIN_COUNT, DRIVE_WARMUP = 0.5, 1, 1
DRIVE_FIGURES = (29, 19, 73, 1861)
DRIVE_LOST_CAP = 93  # a twentieth of the static voxels


def knn_plane_covs(pts, k=20) -> np.ndarray:
    """(n, 4, 4): the covariance of every point's k nearest neighbours (itself among them), its eigenvalues replaced by (1e-3, 1, 1) -
    the plane regularisation, spelled in numpy so that the model and the engine are handed the same numbers (setSourceCovariances)."""
    p = np.asarray(pts, np.float64)
    n = len(p)
    out = np.zeros((n, 4, 4))
    sq = (p * p).sum(axis=1)
    for at in range(0, n, 1024):
        rows = p[at:at + 1024]
        d = sq[at:at + 1024, None] - 2.0 * rows @ p.T + sq[None, :]
        nb = p[np.argpartition(d, k - 1, axis=1)[:, :k]]  # (rows, k, 3)
        c = nb - nb.mean(axis=1, keepdims=True)
        w, V = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c) / k)  # ascending eigenvalues
        out[at:at + 1024, :3, :3] = np.einsum("nij,j,nkj->nik", V, np.array([1e-3, 1.0, 1.0]), V)
    return out


@functools.lru_cache(maxsize=None)
def drive_frames():
    """-> [(pose float32 (4, 4), points float32 (n, 3) in the sensor frame, covariances (n, 4, 4))] for frames 0 .. 6"""
    import _vgicp_ray_drive as drive
    out = []
    for pose, pts, _ in drive.frames()[:DRIVE_FRAMES]:
        p = np.ascontiguousarray(pts[::DRIVE_STRIDE, :3], dtype=np.float32)
        out.append((pose, p, knn_plane_covs(p)))
    return out


def drive_model(max_mahalanobis, min_voxel_count, warmup, K=DRIVE_K, **options):
    """(the map every frame is inserted into ungated, the map whose frames from `warmup` on go through the gate, the gate's results)"""
    plain, gated, results = rm.RollingVoxelMap(DRIVE_RES), rm.RollingVoxelMap(DRIVE_RES), []
    for f, (pose, pts, cv) in enumerate(drive_frames()):
        plain.insert(pts, cv, pose)
        if f < warmup:
            gated.insert(pts, cv, pose)
        else:
            results.append(gated_insert(gated, pts, cv, pose, K, max_mahalanobis, min_voxel_count=min_voxel_count, **options))
    return plain, gated, results


def drive_figures(plain, gated):
    """-> (trail voxels in the ungated map, in the gated one, static voxels of the ungated map that the gated one lacks, static voxels)"""
    import _vgicp_ray_drive as drive
    tp, tg = drive.trail_mask(plain.ijk, DRIVE_RES), drive.trail_mask(gated.ijk, DRIVE_RES)
    have = set(map(tuple, gated.ijk.tolist()))
    lost = sum(1 for key, t in zip(map(tuple, plain.ijk.tolist()), tp) if not t and key not in have)
    return int(tp.sum()), int(tg.sum()), lost, int((~tp).sum())
