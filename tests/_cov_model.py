"""Definition model of the per-point covariance (numpy, float64) and the input families that take the covariance kernel to its
edges: exactly degenerate neighbourhoods, k = 1 and 2, tiny clouds, coordinates far from the origin.

Shared by tests/test_cov_model_cpu.py (the oracle against this model, and the caps that keep the GPU test honest) and
tests/test_gpu_covariances_edges.py (the HIP kernel against the oracle, judged by the same `check_case`).

What is compared by VALUE and what by PROPERTY ("well defined", per regularisation):
  NONE, FROBENIUS, MIN_EIG   always by value.
  NORMALIZED_MIN_EIG         by value; a rank-0 neighbourhood (|w|max == 0) is pinned to 1e-3 * I (include/ngicp.h).
  PLANE                      by value on rows with |w|mid - |w|min > PLANE_GAP * |w|max.  PLANE's output moves by about eps / gap
                             for a perturbation eps of C; eps is about 1e-16 |w|max from rounding and the tolerance is 1e-9, so a
                             relative gap of 1e-6 leaves a factor of 10.  On the other rows (rank <= 1: lines, k <= 2, coincident
                             points) the smallest eigenspace has more than one dimension and any normal inside it is a right
                             answer: `plane_property_errors` checks what every right answer shares.
"""
import functools

import numpy as np

REGS = {"NONE": 0, "MIN_EIG": 1, "NORMALIZED_MIN_EIG": 2, "PLANE": 3, "FROBENIUS": 4}
KS = (1, 2, 3, 10, 20, 32)
TOL = 1e-9          # the project's covariance tolerance (test_gpu_parity.py::test_covariances_match_oracle)
PLANE_GAP = 1e-6    # relative separation of the two smallest |w| above which PLANE is compared by value
AMBIGUOUS_CAP = 0.01
PLANE_SKIP_CAP = 0.02
SEED = 20


# ------------------------------------------------------------------------------------------------ the definition
def raw_covariances(pts, nbr_idx):
    """C = X^T X / k of the mean-centred float32 neighbours, in float64: (n, 3, 3), and its |eigenvalues| ascending: (n, 3)."""
    X = np.asarray(pts, np.float32)[:, :3][nbr_idx].astype(np.float64)  # (n, k, 3)
    X = X - X.mean(axis=1, keepdims=True)
    C = np.einsum("nkr,nkc->nrc", X, X) / nbr_idx.shape[1]
    return C, np.sort(np.abs(np.linalg.eigvalsh(C)), axis=1)


def model_covariances(pts, nbr_idx, reg):
    """The regularised covariance of every point from its neighbour indices: ((n, 4, 4) with a zero last row and column, sorted |w|).

    Per point: gather the k float32 neighbours, cast to float64, centre, C = X^T X / k.  NONE returns C; FROBENIUS is
    inv(inv(C + 1e-3 I) / ||.||_F) with np.linalg.inv.  The SVD modes use the engine's documented symmetric form V f(|w|) V^T from
    np.linalg.eigh (csrc/ngicp_math.h: for a symmetric matrix U == V), NOT oracle/numpy_model.py's U diag V^T of a real SVD: for a
    zero singular value numpy may return u = -v, which turns the floor 1e-3 into -1e-3; the degenerate clouds here are made of
    zero singular values."""
    reg = int(reg)
    C, absw = raw_covariances(pts, nbr_idx)
    if reg == REGS["NONE"]:
        out = C
    elif reg == REGS["FROBENIUS"]:
        Ci = np.linalg.inv(C + 1e-3 * np.eye(3))
        Ci = Ci / np.sqrt((Ci * Ci).sum(axis=(1, 2)))[:, None, None]
        out = np.linalg.inv(Ci)
    else:
        w, V = np.linalg.eigh(C)
        a = np.abs(w)
        if reg == REGS["MIN_EIG"]:
            f = np.maximum(a, 1e-3)
        elif reg == REGS["NORMALIZED_MIN_EIG"]:
            m = a.max(axis=1, keepdims=True)
            f = np.where(m > 0, np.maximum(a / np.where(m > 0, m, 1.0), 1e-3), 1e-3)
        elif reg == REGS["PLANE"]:
            f = np.ones_like(a)
            f[np.arange(len(a)), a.argmin(axis=1)] = 1e-3
        else:
            raise ValueError(reg)
        out = np.einsum("nre,ne,nce->nrc", V, f, V)
    full = np.zeros((len(C), 4, 4))
    full[:, :3, :3] = out
    return full, absw


def neighbour_sets(orc, pts, k):
    """The oracle tree's k nearest indices of every point: (n, k), and the mask `ambiguous`: (n,).

    A row is ambiguous when its k-th and (k+1)-th float32 squared distances are equal AND the points at that distance do not all
    share the same coordinates: then two exact searches may keep different points and the covariance legitimately differs.  A tie
    among coincident points is not ambiguous: the covariance does not depend on which copy is taken.
    To see every point at the tied distance min(n, k + 8) neighbours are queried.  A tie run that reaches the end of that list has
    not been seen whole: the row is queried again with a list twice as long, until the run ends inside the list or the list is the
    whole cloud (32 coincident copies at k = 10 need it).  No row is called unambiguous on a run that was cut off."""
    pts = np.ascontiguousarray(np.asarray(pts, np.float32)[:, :3])
    n = len(pts)
    tree = orc.OracleTree(pts)
    m = min(n, k + 8)
    idx, d2 = tree.knn(pts, m)
    nbr = np.ascontiguousarray(idx[:, :k])
    ambiguous = np.zeros(n, bool)
    if m == k:  # n == k: there is no (k+1)-th point
        return nbr, ambiguous
    rows = np.flatnonzero(d2[:, k - 1] == d2[:, k])
    idx, d2 = idx[rows], d2[rows]
    while len(rows):
        again = []
        for j, r in enumerate(rows):
            run = d2[j] == d2[j, k - 1]
            if run[-1] and m < n:
                again.append(r)
                continue
            p = pts[idx[j][run]]
            ambiguous[r] = bool(np.any(p != p[0]))
        rows = np.array(again, dtype=np.int64)
        if len(rows):
            m = min(n, 2 * m)
            idx, d2 = tree.knn(pts[rows], m)
    return nbr, ambiguous


# ------------------------------------------------------------------------------------------------ the input families
def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


@functools.lru_cache(maxsize=None)
def families(seed=SEED):
    """name -> float32 cloud (n, 3).  Treat the arrays as read-only: they are shared by every test of a session.

    plane_z / plane_x / plane_y   two random coordinates, the third exactly 1.25: exact zeros in C
    plane_tilted                  a random plane rounded to float32: rank 2 only to rounding
    line_x / line_y / line_z      one random coordinate, the other two constant: rank 1, exact zeros
    line_diag                     t * (1, 1, 1), t float32: exactly collinear after rounding, no zero entry in C
    dups4                         300 random points, each 4 times, shuffled: rank 0 at k <= 4, coplanar sites up to k = 12
    dups_k                        30 sites, each 32 times: rank 0 for every k <= 32
    far                           Gaussian, sigma 0.5 m, offset (4000, -2500, 30): float32 spacing 0.25 to 0.5 mm
    far_utm                       Gaussian, sigma 0.75 m, offset (5e5, 4e6, 100): float32 spacing 0.03 to 0.25 m, heavy quantisation
                                  (it meets both caps on the CPU, so it stays)
    tiny_n{n}                     Gaussian clouds (sigma 0.3 m) with n = k and n = k + 1 for k in {1, 2, 10, 20, 32}
    lidar                         clouds.scan_to_scan(2000).source plus an isotropic jitter of 1 cm, the ordinary control
    The extents are as small as they are so that the oracle stays within half the tolerance of the model under FROBENIUS, and the
    jitter keeps `lidar` under the PLANE cap at k = 3: the measurements are in tests/test_cov_model_cpu.py."""
    from direct_lidar_odometry_amd import clouds
    rng = np.random.default_rng(seed)
    out = {}
    for axis, name in enumerate("xyz"):
        p = rng.uniform(-2.0, 2.0, size=(600, 3))
        p[:, axis] = 1.25
        out["plane_" + name] = _f32(p)
    uv = rng.uniform(-2.0, 2.0, size=(600, 2))
    e1, e2 = np.array([0.8, 0.1, 0.59]), np.array([-0.2, 0.9, 0.38])
    out["plane_tilted"] = _f32(uv[:, :1] * e1 + uv[:, 1:] * e2 + np.array([0.3, -0.7, 1.1]))
    for axis, name in enumerate("xyz"):
        p = np.empty((500, 3))
        p[:] = (0.3, -1.7, 2.5)
        p[:, axis] = rng.uniform(-20.0, 20.0, size=500)
        out["line_" + name] = _f32(p)
    t = _f32(rng.uniform(-3.0, 3.0, size=500))
    out["line_diag"] = np.ascontiguousarray(np.stack([t, t, t], axis=1))
    sites = _f32(rng.uniform(-5.0, 5.0, size=(300, 3)))
    out["dups4"] = np.ascontiguousarray(rng.permutation(np.repeat(sites, 4, axis=0)))
    sites = _f32(rng.uniform(-5.0, 5.0, size=(30, 3)))
    out["dups_k"] = np.ascontiguousarray(rng.permutation(np.repeat(sites, 32, axis=0)))
    out["far"] = _f32(rng.normal(size=(1000, 3)) * 0.5 + np.array([4000.0, -2500.0, 30.0]))
    out["far_utm"] = _f32(rng.normal(size=(1000, 3)) * 0.75 + np.array([5e5, 4e6, 100.0]))
    for n in (1, 2, 3, 10, 11, 20, 21, 32, 33):
        out[f"tiny_n{n}"] = _f32(rng.normal(size=(n, 3)) * 0.3)
    out["lidar"] = _f32(clouds.scan_to_scan(2000).source[:, :3].astype(np.float64) + rng.normal(size=(2000, 3)) * 0.01)
    for v in out.values():
        v.setflags(write=False)
    return out


# The smallest k from which a family's neighbourhoods have rank >= 2 by construction (None: never); the PLANE skip cap applies
# from max(3, that k).  dups4: k >= 9 reaches a third site (two sites of four copies hold 8 points).
RANK2_FROM_K = {"line_x": None, "line_y": None, "line_z": None, "line_diag": None, "dups_k": None, "dups4": 9}
# NONE-mode entries (row, column) that the definition makes exactly zero: the centring of k equal float32 values is exact in FP64
EXACT_ZERO_AXES = {"plane_x": (0,), "plane_y": (1,), "plane_z": (2,), "line_x": (1, 2), "line_y": (0, 2), "line_z": (0, 1)}


def cases(names=None):
    """(family, k) for every family and every k in KS with k <= n."""
    fam = families()
    return [(name, k) for name in (names or fam) for k in KS if k <= len(fam[name])]


@functools.lru_cache(maxsize=None)
def _reference_cached(name, k):
    from oracle import oracle as orc
    pts = families()[name]
    nbr, ambiguous = neighbour_sets(orc, pts, k)
    C, absw = raw_covariances(pts, nbr)
    for a in (nbr, ambiguous, C, absw):
        a.setflags(write=False)
    return nbr, ambiguous, C, absw


def reference(name, k):
    """(neighbour indices, ambiguous mask, C, sorted |w|) of a case: computed once per session, read-only."""
    return _reference_cached(name, int(k))


@functools.lru_cache(maxsize=None)
def oracle_covariances(name, k, reg):
    """The oracle's covariances of a case: computed once per session, read-only."""
    from oracle import oracle as orc
    c = np.ascontiguousarray(orc.covariances(families()[name], int(k), int(reg)))
    c.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------ the judgement
def plane_separated(absw):
    return absw[:, 1] - absw[:, 0] > PLANE_GAP * absw[:, 2]


def value_rows(reg, absw, ambiguous):
    """Rows whose covariance is compared by value: unambiguous neighbour set and a well-defined result (module docstring)."""
    rows = ~ambiguous
    if int(reg) == REGS["PLANE"]:
        rows = rows & plane_separated(absw)
    return rows


def plane_property_errors(out3, C, absw):
    """What every right PLANE answer shares, per row of out3 (m, 3, 3): (asymmetry, eigenvalue error, normal excess).
      asymmetry     max |out - out^T|: must be exactly 0 for the engine (see check_case);
      eigenvalues   distance of the sorted eigenvalues from (1e-3, 1, 1): at most 1e-12;
      normal        n^T C n - |w|min for the 1e-3 eigenvector n, in units of max(|w|max, 1e-300): at most 1e-12.  The normal lies
                    in the smallest eigenspace, so a line's direction keeps variance 1."""
    if len(out3) == 0:
        return 0.0, 0.0, 0.0
    asym = float(np.abs(out3 - out3.transpose(0, 2, 1)).max())
    w, V = np.linalg.eigh(out3)
    eig = float(np.abs(w - np.array([1e-3, 1.0, 1.0])).max())
    nrm = V[:, :, 0]
    excess = (np.einsum("nr,nrc,nc->n", nrm, C, nrm) - absw[:, 0]) / np.maximum(absw[:, 2], 1e-300)
    return asym, eig, float(excess.max())


def check_case(out, ref, name, k, reg, sym_tol=0.0):
    """Judge the (n, 4, 4) covariances `out` of case (name, k, reg) against `ref` (same shape): structure on every row, values to
    TOL on the well-defined unambiguous rows, the PLANE properties on the other unambiguous rows.  Returns the figures.
    sym_tol: allowed |out - out^T| in units of max |out|.  0 for the engine, which stores the six entries of the upper triangle
    once.  The oracle forms all nine entries of V f V^T, and (V[r][e] f[e]) V[c][e] rounds differently from (V[c][e] f[e]) V[r][e]:
    three products of two roundings each and two additions, in either order, stay within 8 eps = 1e-15."""
    reg = int(reg)
    n = len(families()[name])
    _, ambiguous, C, absw = reference(name, k)
    assert out.shape == (n, 4, 4)
    assert np.all(np.isfinite(out)), "non-finite covariance"
    assert np.all(out[:, 3, :] == 0.0) and np.all(out[:, :, 3] == 0.0)
    sym_abs = sym_tol * float(np.abs(out).max())
    assert np.abs(out - out.transpose(0, 2, 1)).max() <= sym_abs, "not symmetric"
    rows = value_rows(reg, absw, ambiguous)
    fig = {"n": n, "value_rows": int(rows.sum()), "ambiguous": float(ambiguous.mean()), "max_diff": 0.0}
    if rows.any():
        fig["max_diff"] = float(np.abs(out - ref)[rows].max())
        assert fig["max_diff"] < TOL, (name, k, reg, fig)
    if reg == REGS["PLANE"]:
        rest = ~ambiguous & ~rows
        fig["plane_property_rows"] = int(rest.sum())
        asym, eig, excess = plane_property_errors(out[rest][:, :3, :3], C[rest], absw[rest])
        fig["plane_property"] = (asym, eig, excess)
        assert asym <= sym_abs and eig <= 1e-12 and excess <= 1e-12, (name, k, fig)
    if reg == REGS["NONE"]:
        if k == 1 or name == "dups_k":
            assert np.all(out[~ambiguous] == 0.0), "a rank-0 neighbourhood has an exactly zero covariance"
        for ax in EXACT_ZERO_AXES.get(name, ()):
            assert np.all(out[~ambiguous][:, ax, :] == 0.0) and np.all(out[~ambiguous][:, :, ax] == 0.0), (name, k, ax)
    if reg == REGS["NORMALIZED_MIN_EIG"]:
        flat = ~ambiguous & (absw[:, 2] == 0.0)
        if flat.any():  # the pinned rule: no ratio is taken, every value gets the floor
            assert np.array_equal(out[flat][:, :3, :3], np.broadcast_to(1e-3 * np.eye(3), (int(flat.sum()), 3, 3)))
    return fig
