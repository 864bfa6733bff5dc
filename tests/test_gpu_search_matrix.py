"""The exact search under the per-handle switches and the grid geometries the default configuration never meets (-m gpu).

The engine's promise is that its nearest-neighbour search is exact at any voxel size and under any switch: float32 squared distances
bit-equal to the oracle's, indices equal except on exact float32 ties.  test_gpu_passes.py checks that on every pass of an alignment,
but only on the paths its workloads happen to take.  Here the same per-pass check (_pass_check.py) runs under:

  * NGICP_STAGE_GROW 0 / 1 / 2 / 6: straight from global memory, no row lists, the shortest list, the default (stats()'s
    staged_fraction shows which ran: queries served through the listed rows of their batch region, ngicp_pass_group.inc in_box);
  * setTuning voxels from one that make_grid has to grow to one cell for the whole cloud;
  * NGICP_TARGET_OCC 1 / 400 (the automatic voxel far smaller / larger than the default);
  * clouds 3.6 km from the origin (Grid::slack's 4e-6 |mn| term);
  * a first pass that lists no rows although many of its queries look far (the handle's previous alignment served < 12 % of its
    queries through lists, ngicp_api.hip do_align).

The query entry points (k-NN on both index slots, radiusSearch, fitness, the covariance k-NN) are compared with numpy brute force in the
engine's association on a lattice whose points and queries lie exactly on cell faces, clusters with empty cells between them, a cloud
of zero extent on two axes and a cloud 3.6 km from the origin, at voxels from 0.02 (grown by make_grid) to 1000 (one cell), with queries
up to 10^4 times the cloud's extent outside the grid (clamped to its border cells)."""
import numpy as np
import pytest

from direct_lidar_odometry_amd import clouds
from direct_lidar_odometry_amd.nano_gicp import FLT_MAX

from _pass_check import CASES, FIXED20, REJECTION_GUESS, SHAPES, Rig, make_rig
from test_gpu_parity import _boundary_ties
from test_gpu_queries import DBL_MAX, _check_fitness, _check_radius, _d2_rows, _nn_d2, _transformed

pytestmark = pytest.mark.gpu

MAX_CELLS = 1 << 25  # make_grid's caps (ngicp_api.hip): cells, and rows packed as y | z << 16
FAR = np.array([3000.0, -2000.0, 50.0])


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _caps(s):
    nx, ny, nz = s["grid_dims"]
    assert min(nx, ny, nz) >= 1 and nx * ny * nz <= MAX_CELLS and ny < 65536 and nz < 32768, s["grid_dims"]


# ------------------------------------------------------------------ NGICP_STAGE_GROW
GROW_CASES = [(case, grow) for grow in ("0", "1", "2", "6") for case in ("dlo_s2s", "fixed20", "gauss_newton", "lm_rejection", "lines", "clumps")]
GROW_CASES += [("c3_fixed20", "0"), ("c3_fixed20", "1")]


@pytest.mark.parametrize("case,grow", GROW_CASES, ids=[f"{c}-grow{g}" for c, g in GROW_CASES])
def test_every_pass_under_stage_grow(ng, oracle_mod, case, grow):
    """0: every query searches straight from global memory; 1: no row lists (listing needs stage_grow >= 2), so the shell walk in
    global memory serves every query that looks past ring 1; 2: the shortest list; 6: the default."""
    rig, guess = make_rig(ng, oracle_mod, case, env={"NGICP_STAGE_GROW": grow})
    rig.run(guess, f"{case} NGICP_STAGE_GROW={grow}")
    first = rig.first_align_stats(guess)["staged_fraction"]
    last = rig.g.stats()["staged_fraction"]
    print(f"{case} grow {grow}: staged fraction {first:.4f} (first alignment), {last:.4f} (last)")
    if grow in ("0", "1"):
        assert first == 0.0 and last == 0.0
    elif case in ("lm_rejection", "lines", "clumps"):  # far starts: regions small enough to list (the good guesses' may not be)
        assert first > 0.0


# ------------------------------------------------------------------ voxel sizes
@pytest.mark.parametrize("voxel", [0.02, 0.5, 3.0, 1000.0])
@pytest.mark.parametrize("case", ["dlo_s2s", "lm_rejection", *SHAPES])
def test_every_pass_voxel_sizes(ng, oracle_mod, case, voxel):
    """0.02: more cells than make_grid allows on most of these clouds (it grows the voxel); 0.5 / 3.0: cells up to three times the
    gate; 1000: one cell, every pass a brute force."""
    rig, guess = make_rig(ng, oracle_mod, case, tuning=voxel)
    rig.run(guess, f"{case} voxel {voxel}")
    s = rig.g.stats()
    h, dims = s["voxel_size"], s["grid_dims"]
    print(f"{case} voxel {voxel}: h {h}, grid {dims}")
    _caps(s)
    assert h >= np.float32(voxel)
    if h > np.float32(voxel):  # grown (stats() reports the target's grid): only because the edge before broke a cap
        n = np.floor(np.ptp(rig.tgt[:, :3].astype(np.float64), 0) / (h / 1.26)) + 1
        assert n.prod() > MAX_CELLS or n[1] >= 65536 or n[2] >= 32768, (h, dims)
    if voxel == 0.02 and case in ("dlo_s2s", "lm_rejection", "lines"):
        assert h > 0.02
    if voxel == 1000.0:
        assert dims == [1, 1, 1]


# ------------------------------------------------------------------ NGICP_TARGET_OCC
@pytest.mark.parametrize("occ", ["1", "400"])
@pytest.mark.parametrize("case", ["dlo_s2s", "c3_dlo"])
def test_every_pass_target_occupancy(ng, oracle_mod, case, occ):
    rig, guess = make_rig(ng, oracle_mod, case, env={"NGICP_TARGET_OCC": occ})
    rig.run(guess, f"{case} NGICP_TARGET_OCC={occ}")
    d = ng.NanoGICP()  # the default handle on the same clouds
    d.setInputSource(rig.src); d.setInputTarget(rig.tgt)
    d.setSourceCovariances(rig.cs); d.setTargetCovariances(rig.ct)
    d.setMaximumIterations(1)
    d.align(np.asarray(guess, np.float32))
    h, h_default = rig.g.stats()["voxel_size"], d.stats()["voxel_size"]
    d.close()
    print(f"{case} occupancy {occ}: voxel {h} (default {h_default})")
    assert (h < h_default) if occ == "1" else (h > h_default)


# ------------------------------------------------------------------ far from the origin
def _shifted(T, s):
    S = np.eye(4)
    S[:3, 3] = s
    return (S @ np.asarray(T, np.float64) @ np.linalg.inv(S)).astype(np.float32)


@pytest.mark.parametrize("tuning", [None, 0.25])
def test_every_pass_far_from_origin(ng, oracle_mod, tuning):
    """The 10k scan-to-scan with both clouds 3.6 km from the origin and the guess conjugated by the shift.  A float32 coordinate there
    has a 2.4e-4 m ulp: the grid's cell assignment and face distances round by that much, which Grid::slack's 4e-6 |mn| term covers.
    The correspondences must be bit-exact and H within H_TOL as everywhere; the LM trace's y0 / yi, which the GPU evaluates at the double
    pose and the oracle at double(float(pose)), within H_TOL plus the bound of that rounding (_pass_check.pose_rounding_bound: up to
    ~1e-4 of the error on the converged passes here, against ~1e-7 near the origin)."""
    w = clouds.scan_to_scan(10_000)
    src = np.ascontiguousarray((w.source[:, :3].astype(np.float64) + FAR).astype(np.float32))
    tgt = np.ascontiguousarray((w.target[:, :3].astype(np.float64) + FAR).astype(np.float32))
    settings, gate = CASES["dlo_s2s"]
    settings = dict(settings)
    k = settings.pop("setCorrespondenceRandomness")
    rig = Rig(ng, oracle_mod, src, tgt, k, gate, settings, tuning=tuning)
    out = rig.run(_shifted(w.guess, FAR), f"far from the origin, voxel {tuning}", pose_rounding=True)
    assert len(out) >= 2
    if tuning is not None:
        assert rig.g.stats()["voxel_size"] == np.float32(tuning)


# ------------------------------------------------------------------ a first pass that lists no rows
def test_every_pass_first_pass_without_row_lists(ng, oracle_mod):
    """Whether an alignment's first pass lists region rows depends on the handle's previous alignment (>= 12 % of its queries served
    through lists).  Before every alignment checked here, the same handle runs a FIXED20 alignment from the good guess with a small
    gate, which serves fewer than that; the alignment checked then starts from REJECTION_GUESS without a gate, where many queries look far."""
    w = clouds.scan_to_scan(10_000)
    rig = Rig(ng, oracle_mod, w.source, w.target, 20, None, FIXED20)
    fractions = []

    def prime(g, n):  # a 5 cm gate: after its first pass no batch looks beyond ring 1, so 20 passes serve < 12 % through lists
        g.setMaximumIterations(20)
        g.setMaxCorrespondenceDistance(0.05)
        g.align(w.guess)
        s = g.stats()
        assert s["passes"] > 1 and s["staged_fraction"] < 0.12, (s["passes"], s["staged_fraction"])
        fractions.append(s["staged_fraction"])
        g.setMaximumIterations(n)
        g.setMaxCorrespondenceDistance(FLT_MAX)  # (the rig's gate: none)

    out = rig.run(REJECTION_GUESS, "first pass without row lists", prime=prime)
    print(f"staged fractions of the priming alignments: {min(fractions):.4f} .. {max(fractions):.4f}; passes checked {len(out)}")
    assert len(out) >= 2


# ------------------------------------------------------------------ the query entry points
def _lattice():
    """0.25 m lattice from the origin (exactly representable), 200 points duplicated."""
    ax, az = np.arange(16) * 0.25, np.arange(8) * 0.25
    pts = np.stack(np.meshgrid(ax, ax, az, indexing="ij"), -1).reshape(-1, 3)
    dup = pts[np.random.default_rng(5).choice(len(pts), 200, replace=False)]
    return np.r_[pts, dup]


def _clusters():
    rng = np.random.default_rng(6)
    centres = rng.uniform(-10, 10, (8, 3))
    return centres[rng.integers(0, 8, 2400)] + 0.05 * rng.standard_normal((2400, 3))


def _flat():
    """zero extent along y and z"""
    x = np.random.default_rng(7).uniform(-10, 10, 2000)
    return np.c_[x, np.full(2000, 1.5), np.full(2000, -0.5)]


def _far():
    return np.random.default_rng(8).uniform(-4, 4, (3000, 3)) + FAR


QUERY_CLOUDS = {"lattice": _lattice, "clusters": _clusters, "flat": _flat, "far": _far}
QUERY_POSE = clouds.make_pose((0.05, -0.03, 0.02), (1.0, -2.0, 3.0))


def _queries(pts, h, rng):
    """Transformed cloud points; points with one to three coordinates snapped exactly onto the grid's cell faces (origin = the cloud's
    float minimum, faces at ox + i * h in float32, as the kernels compute them); points 10^2 .. 10^4 extents away along the axes and
    the diagonals."""
    n = len(pts)
    mn = pts.min(0)
    T = np.asarray(_shifted(QUERY_POSE, pts.mean(0)), np.float64)
    moved = (pts[rng.choice(n, 300, replace=False)].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    snap = pts[rng.choice(n, 240, replace=False)].copy()
    hf = np.float32(h)
    for i, p in enumerate(snap):
        for a in range(3):
            if (i >> a) & 1 or i % 8 == 0:
                cell = np.floor((np.float64(p[a]) - np.float64(mn[a])) / np.float64(hf) + 0.5)
                snap[i, a] = np.float32(mn[a] + np.float32(cell) * hf)
    ext = max(float(np.ptp(pts.astype(np.float64), 0).max()), 1.0)
    dirs = [np.eye(3)[a] * s for a in range(3) for s in (1, -1)]
    dirs += [np.array([sx, sy, sz]) / np.sqrt(3.0) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    c = pts.astype(np.float64).mean(0)
    far = np.array([c + d * f * ext for d in dirs for f in (1e2, 1e3, 1e4)], np.float32)
    return np.ascontiguousarray(np.concatenate([moved, snap, far]).astype(np.float32)), len(moved) + len(snap)


def _check_knn(g, which, pts, q, D, k):
    """distances bit-equal to the k smallest of the brute-force row; every index valid, distinct and at exactly its reported distance
    (so the indices strictly closer than the k-th distance are exactly the brute force's; only the k-th distance's ties are free)."""
    gi, gd = g.nearestKSearch(q, k, which=which)
    ref = np.sort(np.partition(D, k - 1, axis=1)[:, :k], axis=1)  # the k smallest of every row, ascending (as np.sort(D, axis=1)[:, :k], without sorting the rest)
    bad = np.flatnonzero((gd != ref).any(1))
    assert not len(bad), f"{which} k {k}: query {bad[0]} {q[bad[0]]}: d2 {gd[bad[0]]} vs {ref[bad[0]]} ({len(bad)} queries)"
    assert gi.min() >= 0 and gi.max() < len(pts)
    own = np.take_along_axis(D, gi.astype(np.int64), 1)
    bad = np.flatnonzero((own != gd).any(1))
    assert not len(bad), f"{which} k {k}: query {bad[0]}: indices {gi[bad[0]]} are at {own[bad[0]]}, not {gd[bad[0]]}"
    s = np.sort(gi, 1)
    assert np.all(s[:, 1:] != s[:, :-1]), f"{which} k {k}: an index twice in one row"
    kth = gd[:, -1:]
    assert np.array_equal((D < kth).sum(1), (gd < kth).sum(1))


@pytest.mark.parametrize("voxel", [0.0, 0.02, 0.25, 1000.0], ids=["auto", "0.02", "0.25", "1000"])
@pytest.mark.parametrize("cloud", list(QUERY_CLOUDS))
def test_queries_under_grid_geometries(ng, oracle_mod, cloud, voxel):
    pts = np.ascontiguousarray(QUERY_CLOUDS[cloud]().astype(np.float32))
    g = ng.NanoGICP()
    g.setTuning(voxel)
    g.setMaxCorrespondenceDistance(1.0)
    g.setInputSource(pts); g.setInputTarget(pts)
    g.setMaximumIterations(1)
    g.align()  # (stats() reports the grid of the last alignment)
    s = g.stats()
    h = s["voxel_size"]
    _caps(s)
    if voxel > 0:
        assert h >= np.float32(voxel)
    if voxel == 1000.0:
        assert s["grid_dims"] == [1, 1, 1]
    if cloud == "lattice" and voxel == 0.25:
        assert h == 0.25 and s["grid_dims"] == [16, 16, 8]  # the lattice's points lie on the cell faces
    rng = np.random.default_rng(int(voxel * 100) + len(cloud))
    q, n_near = _queries(pts, h, rng)
    D = _d2_rows(pts, q)
    print(f"{cloud} voxel {voxel}: h {h}, grid {s['grid_dims']}, {len(pts)} points, {len(q)} queries")
    for which in ("source", "target"):
        for k in (1, 7, 20, 32):
            _check_knn(g, which, pts, q, D, k)
        for radius in ((0.4 * h) ** 2, (2.5 * h) ** 2):
            _check_radius(g, which, pts, q, radius)
    # fitness: the source under a pose, searched in the target index
    T = _shifted(QUERY_POSE, pts.mean(0))
    d2 = _nn_d2(pts, _transformed(g, oracle_mod, pts, T))
    for max_range in (DBL_MAX, (0.5 * h) ** 2):
        _check_fitness(g, d2, max_range, T)
    # the covariance k-NN on the source index, away from k-th neighbour ties (test_covariances_match_oracle)
    g.calculateSourceCovariances()
    _check_covariances(oracle_mod, pts, g.getSourceCovariances())
    g.close()


def _check_covariances(orc, pts, a, k=20):
    """a: the GPU's covariances of pts (k neighbours, plane regularisation) against the oracle's, away from k-th neighbour ties.  The
    regularisation is C = I - (1 - 1e-3) u u^T, u the eigenvector of the smallest eigenvalue of the neighbours' raw covariance; where the
    two smallest are equal (a symmetric lattice neighbourhood, the two empty axes of a line) u is any vector of their plane, in the
    oracle as on the GPU, and only what does not depend on it is compared: C v for the eigenvector v of a distinct largest eigenvalue,
    and C's eigenvalues.  Returns the number of points compared in full."""
    b = orc.covariances(pts, k)
    ties = _boundary_ties(orc, pts, k)
    idx, _ = orc.OracleTree(pts).knn(pts, k)
    nb = pts[idx.astype(np.int64)].astype(np.float64)
    nb -= nb.mean(1, keepdims=True)
    lam, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", nb, nb) / k)
    scale = np.maximum(lam[:, 2], 1e-30)
    free = lam[:, 1] - lam[:, 0] <= 1e-5 * scale
    full = ~ties & ~free
    if full.any():
        assert np.abs(a - b)[full].max() < 1e-9
    part = ~ties & free
    v = vec[:, :, 2]
    axis = part & (lam[:, 2] - lam[:, 1] > 1e-5 * scale)
    if axis.any():
        Av, Bv = (np.einsum("nij,nj->ni", c[axis, :3, :3], v[axis]) for c in (a, b))
        assert np.abs(Av - Bv).max() < 1e-9
    if part.any():
        assert np.abs(np.linalg.eigvalsh(a[part, :3, :3]) - np.linalg.eigvalsh(b[part, :3, :3])).max() < 1e-9
    print(f"covariances: {int(full.sum())} compared in full, {int(axis.sum())} along their axis, {int(part.sum())} by eigenvalues, {int(ties.sum())} ties")
    return int(full.sum())
