"""The numpy model of the pose graph (include/ngicp.h, "pose graph").   *** TEST INFRASTRUCTURE ONLY ***

The definition is the project's own, so the model proves itself (tests/test_pose_graph_model_cpu.py: Jacobians against central
differences, the optimiser against ground truth, edge_from_alignment against its third-order rule) and the engine is held to the
model (tests/test_gpu_pose_graph.py).  Everything is float64 and vectorised over edges.  Not collected by pytest (no test_ prefix).

  nodes      T_k = (R_k, t_k), 4x4; `fixed` flags
  edges      (i, j, Z, Lambda, robust flag);  E = Z^-1 T_i^-1 T_j,  r = (so3_log(R_E), t_E),  s = r^T Lambda r
  update     T_k <- (so3_exp(d[0:3]), d[3:6]) * T_k
  Jacobians  with A = Z^-1 T_i^-1:   J_j = [[Jl^-1(phi) R_A, 0], [-R_A [t_j]x, R_A]],   J_i = [[-Jl^-1(phi) R_A, 0], [R_A [t_j]x, -R_A]]
  cost       chi2 = sum rho(s_e); rho, w from tests/_robust_model.rho_w for flagged edges when a kernel is chosen, identity otherwise
  LM         csrc/ngicp_lm.h's schedule on the whole graph (optimize below)
"""
from __future__ import annotations

import numpy as np

import _robust_model as rm

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = rm.NONE, rm.HUBER, rm.CAUCHY, rm.GEMAN_MCCLURE
LOG_TAYLOR_S2 = 1e-6
JINV_TAYLOR_TH2 = 1e-2
MAX_NODES, MAX_EDGES = 1 << 20, 1 << 22      # ngpg::kMaxNodes, kMaxEdges
TRACE_CAP = 256                              # NGICP_PG_TRACE_CAP
LM_MAX_TRIES = 10                            # the inner tries of step_lm
LM_INIT_LAMBDA_FACTOR = 1e-9
DEFAULTS = dict(max_iterations=64, rot_eps=2e-3, trans_eps=5e-4, cg_tol=1e-8, cg_max_iterations=1000)


class Refused(ValueError):
    """a call the header answers with NGICP_ERR_ARG; the graph is as it was"""


# ---------------------------------------------------------------- SO(3), batched
def skew(v):
    v = np.asarray(v, np.float64)
    S = np.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -v[..., 2], v[..., 1]
    S[..., 1, 0], S[..., 1, 2] = v[..., 2], -v[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -v[..., 1], v[..., 0]
    return S


def so3_exp(w):
    """so3_exp_matrix of csrc/ngicp_math.h: the quaternion, then its matrix without normalisation.  (..., 3) -> (..., 3, 3)"""
    w = np.asarray(w, np.float64)
    th2 = np.sum(w * w, axis=-1)
    small = th2 < 1e-10
    th = np.sqrt(np.where(small, 1.0, th2))
    imag = np.where(small, 0.5 - th2 / 48.0 + th2 * th2 / 3840.0, np.sin(0.5 * th) / th)
    real = np.where(small, 1.0 - th2 / 8.0 + th2 * th2 / 384.0, np.cos(0.5 * th))
    qx, qy, qz = imag * w[..., 0], imag * w[..., 1], imag * w[..., 2]
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz = tx * real, ty * real, tz * real
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    R = np.empty(w.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - (tyy + tzz), txy - twz, txz + twy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = txy + twz, 1 - (txx + tzz), tyz - twx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = txz - twy, tyz + twx, 1 - (txx + tyy)
    return R


def so3_log(R):
    """so3_log of csrc/ngicp_math.h, valid to 3 rad.  (..., 3, 3) -> (..., 3)"""
    R = np.asarray(R, np.float64)
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    c = 0.5 * ((R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]) - 1.0)
    s2 = np.sum(v * v, axis=-1)
    series = (s2 < LOG_TAYLOR_S2) & (c > 0.0)
    s = np.sqrt(s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        f_trig = np.where(s > 0.0, np.arctan2(s, c) / np.where(s > 0.0, s, 1.0), 0.0)
    f = np.where(series, 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0 + s2 * (15.0 / 336.0))), f_trig)
    return f[..., None] * v


def jinv_coeff(th2):
    th2 = np.asarray(th2, np.float64)
    series = 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0 + th2 * (1.0 / 1209600.0 + th2 * (1.0 / 47900160.0))))
    safe = np.where(th2 < JINV_TAYLOR_TH2, 1.0, th2)
    half = 0.5 * np.sqrt(safe)
    return np.where(th2 < JINV_TAYLOR_TH2, series, (1.0 - half * np.cos(half) / np.sin(half)) / safe)


def left_jacobian_inv(phi):
    """J_l^-1(phi) = I - [phi]x / 2 + c(theta) (phi phi^T - theta^2 I).  (..., 3) -> (..., 3, 3)"""
    phi = np.asarray(phi, np.float64)
    th2 = np.sum(phi * phi, axis=-1)
    eye = np.eye(3)
    return (eye - 0.5 * skew(phi)) + jinv_coeff(th2)[..., None, None] * (phi[..., :, None] * phi[..., None, :] - th2[..., None, None] * eye)


def make_pose(w, t):
    T = np.eye(4)
    T[:3, :3] = so3_exp(np.asarray(w, np.float64))
    T[:3, 3] = t
    return T


def inv_pose(T):
    T = np.asarray(T, np.float64)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum("...ij,...j->...i", Rt, T[..., :3, 3])
    out[..., 3, 3] = 1.0
    return out


def left_update(d, T):
    """(so3_exp(d[0:3]), d[3:6]) * T, batched"""
    d, T = np.asarray(d, np.float64), np.asarray(T, np.float64)
    D = np.zeros(d.shape[:-1] + (4, 4))
    D[..., :3, :3] = so3_exp(d[..., :3])
    D[..., :3, 3] = d[..., 3:]
    D[..., 3, 3] = 1.0
    return D @ T


# ---------------------------------------------------------------- the graph
class Graph:
    def __init__(self):
        self.poses = np.zeros((0, 4, 4))
        self.fixed = np.zeros(0, bool)
        self.ij = np.zeros((0, 2), np.int64)
        self.Z = np.zeros((0, 4, 4))
        self.info = np.zeros((0, 6, 6))
        self.flags = np.zeros(0, bool)
        self.kind, self.width = NONE, 1.0

    def copy(self):
        g = Graph()
        for k in ("poses", "fixed", "ij", "Z", "info", "flags"):
            setattr(g, k, getattr(self, k).copy())
        g.kind, g.width = self.kind, self.width
        return g

    @property
    def n(self):
        return len(self.poses)

    @property
    def m(self):
        return len(self.ij)

    def add_nodes(self, T, fixed=None):
        T = check_add_nodes(self.n, T)
        first = self.n
        self.poses = np.concatenate([self.poses, T])
        self.fixed = np.concatenate([self.fixed, np.zeros(len(T), bool) if fixed is None else np.asarray(fixed, bool)])
        return first

    def add_edges(self, ij, Z, info, flags=None):
        ij, Z, info = check_add_edges(self.n, self.m, ij, Z, info)
        first = self.m
        self.ij = np.concatenate([self.ij, ij])
        self.Z = np.concatenate([self.Z, Z])
        self.info = np.concatenate([self.info, info])
        self.flags = np.concatenate([self.flags, np.zeros(len(ij), bool) if flags is None else np.asarray(flags, bool)])
        return first


def check_add_nodes(n_now, T):
    """everything an add of nodes refuses, all or nothing; -> the poses as (n, 4, 4)"""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    if len(T) == 0:
        raise Refused("n == 0")
    if n_now + len(T) > MAX_NODES:
        raise Refused("node cap")
    check_poses(T, "node")
    return T


def check_add_edges(n_nodes, m_now, ij, Z, info):
    """everything an add of edges refuses, all or nothing; -> (ij, Z, info) as arrays"""
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    Z = np.asarray(Z, np.float64).reshape(-1, 4, 4)
    info = np.asarray(info, np.float64).reshape(-1, 6, 6)
    if len(ij) == 0:
        raise Refused("n == 0")
    if m_now + len(ij) > MAX_EDGES:
        raise Refused("edge cap")
    if ((ij < 0) | (ij >= n_nodes)).any():
        raise Refused("unknown node id")
    if (ij[:, 0] == ij[:, 1]).any():
        raise Refused("self-edge")
    check_poses(Z, "Z")
    if not np.isfinite(info).all():
        raise Refused("information not finite")
    if not np.array_equal(info, np.swapaxes(info, 1, 2)):
        raise Refused("information not symmetric (mirrored entries must be equal)")
    return ij, Z, info


def check_poses(T, what):
    if not np.isfinite(T).all():
        raise Refused(f"{what}: an entry is not finite")
    if not (T[:, 3] == np.array([0.0, 0.0, 0.0, 1.0])).all():
        raise Refused(f"{what}: last row is not (0, 0, 0, 1)")


# ---------------------------------------------------------------- the plan: union-find components, CSR
def components(n, ij):
    """-> root[n] with the union-find the plan header runs: union by smaller root id, full path compression.  The labels themselves are
    not part of the definition; only which nodes share one is."""
    parent = list(range(n))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r
    for a, b in np.asarray(ij, np.int64).reshape(-1, 2):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(a) for a in range(n)], np.int64)


def ungauged_components(n, ij, fixed):
    """number of connected components that hold no fixed node"""
    root = components(n, ij)
    has = np.zeros(n, bool)
    has[root[np.asarray(fixed, bool)]] = True
    return int(sum(1 for r in np.unique(root) if not has[r])) if n else 0


def csr(n, ij):
    """-> (offsets[n + 1], entries[2 m]) with entry = 2 * edge + side (side 0: the node is the edge's i, 1: its j), per node in ascending
    edge id"""
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    lists = [[] for _ in range(n)]
    for e, (a, b) in enumerate(ij):
        lists[a].append(2 * e)
        lists[b].append(2 * e + 1)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([v for l in lists for v in l], np.int64)


# ---------------------------------------------------------------- residuals, Jacobians, linearisation
def edge_frames(Ti, Tj, Z):
    """-> (R_A, R_E, t_E) with A = Z^-1 T_i^-1, E = A T_j"""
    A = inv_pose(Z) @ inv_pose(Ti)
    E = A @ Tj
    return A[..., :3, :3], E[..., :3, :3], E[..., :3, 3]


def residual(Ti, Tj, Z):
    _, RE, tE = edge_frames(np.asarray(Ti, np.float64), np.asarray(Tj, np.float64), np.asarray(Z, np.float64))
    return np.concatenate([so3_log(RE), tE], axis=-1)


def jacobians(Ti, Tj, Z):
    """-> (r, J_i, J_j): analytic, exact at d = 0, under the project's perturbation of T_i and of T_j"""
    Ti, Tj, Z = (np.asarray(a, np.float64) for a in (Ti, Tj, Z))
    RA, RE, tE = edge_frames(Ti, Tj, Z)
    phi = so3_log(RE)
    r = np.concatenate([phi, tE], axis=-1)
    P = left_jacobian_inv(phi) @ RA
    Q = RA @ skew(Tj[..., :3, 3])
    Jj = np.zeros(r.shape[:-1] + (6, 6))
    Jj[..., :3, :3], Jj[..., 3:, :3], Jj[..., 3:, 3:] = P, -Q, RA
    Ji = np.zeros_like(Jj)
    Ji[..., :3, :3], Ji[..., 3:, :3], Ji[..., 3:, 3:] = -P, Q, -RA
    return r, Ji, Jj


class Lin:
    """a linearisation: per-edge r, s, rho, w and blocks; per-node gradient and diagonal blocks (zero for fixed nodes)"""


def cost(g, poses=None):
    poses = g.poses if poses is None else poses
    if g.m == 0:
        return 0.0
    r = residual(poses[g.ij[:, 0]], poses[g.ij[:, 1]], g.Z)
    s = np.einsum("ei,eij,ej->e", r, g.info, r)
    rho, _ = rm.rho_w(s, g.kind, g.width)
    return float(np.sum(np.where(g.flags, rho, s)))


def linearize(g, poses=None):
    poses = g.poses if poses is None else poses
    L = Lin()
    n, m = g.n, g.m
    i, j = g.ij[:, 0], g.ij[:, 1]
    L.r, Ji, Jj = jacobians(poses[i], poses[j], g.Z) if m else (np.zeros((0, 6)), np.zeros((0, 6, 6)), np.zeros((0, 6, 6)))
    L.s = np.einsum("ei,eij,ej->e", L.r, g.info, L.r)
    rho, w = rm.rho_w(L.s, g.kind, g.width)
    L.rho, L.w = np.where(g.flags, rho, L.s), np.where(g.flags, w, 1.0)
    L.chi2 = float(np.sum(L.rho))
    W = L.w[:, None, None] * g.info
    WJi, WJj, Wr = W @ Ji, W @ Jj, np.einsum("eij,ej->ei", W, L.r)
    JiT, JjT = np.swapaxes(Ji, 1, 2), np.swapaxes(Jj, 1, 2)
    L.Hii, L.Hij, L.Hjj = JiT @ WJi, JiT @ WJj, JjT @ WJj
    L.bi, L.bj = np.einsum("eij,ej->ei", JiT, Wr), np.einsum("eij,ej->ei", JjT, Wr)
    L.grad, L.diag = np.zeros((n, 6)), np.zeros((n, 6, 6))
    np.add.at(L.grad, i, L.bi)
    np.add.at(L.grad, j, L.bj)
    np.add.at(L.diag, i, L.Hii)
    np.add.at(L.diag, j, L.Hjj)
    L.grad[g.fixed] = 0.0
    L.diag[g.fixed] = 0.0
    L.fixed = g.fixed.copy()
    L.ij = g.ij
    return L


def system_matrix(L):
    """-> the sparse 6n x 6n H with the rows and columns of fixed nodes zero (scipy CSR)"""
    import scipy.sparse as sp
    n = len(L.fixed)
    i, j = L.ij[:, 0], L.ij[:, 1]
    a = np.arange(6)
    rows, cols, vals = [], [], []

    def put(bi, bj, B):
        keep = ~(L.fixed[bi] | L.fixed[bj])
        rr = (6 * bi[keep, None, None] + a[None, :, None]) + 0 * a[None, None, :]
        cc = (6 * bj[keep, None, None] + a[None, None, :]) + 0 * a[None, :, None]
        rows.append(rr.ravel()), cols.append(cc.ravel()), vals.append(B[keep].ravel())
    put(i, i, L.Hii), put(i, j, L.Hij), put(j, i, np.swapaxes(L.Hij, 1, 2)), put(j, j, L.Hjj)
    if not rows:
        return sp.csr_matrix((6 * n, 6 * n))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n))


def multiply(L, lam, x):
    """(H + lam I) x over the free nodes; rows of fixed nodes are zero and their x is not read"""
    x = np.asarray(x, np.float64).reshape(-1, 6).copy()
    x[L.fixed] = 0.0
    y = (system_matrix(L) @ x.ravel()).reshape(-1, 6) + lam * x
    y[L.fixed] = 0.0
    return y


def _free_index(fixed):
    free = np.flatnonzero(~fixed)
    return (6 * free[:, None] + np.arange(6)[None, :]).ravel()


DENSE_LIMIT = 1800  # unknowns up to which the direct solve is np.linalg.solve; a sparse direct factorisation (scipy spsolve) beyond


def solve_direct(L, lam):
    """delta (n, 6) with (H + lam I) delta = -b on the free nodes, by a direct solve"""
    idx = _free_index(L.fixed)
    out = np.zeros(6 * len(L.fixed))
    if len(idx) == 0:
        return out.reshape(-1, 6), 0
    A = system_matrix(L)[idx][:, idx]
    rhs = -L.grad.ravel()[idx]
    if len(idx) <= DENSE_LIMIT:
        out[idx] = np.linalg.solve(A.toarray() + lam * np.eye(len(idx)), rhs)
    else:
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve
        out[idx] = spsolve((A + lam * sp.identity(len(idx))).tocsc(), rhs)
    return out.reshape(-1, 6), 0


def solve_pcg(L, lam, cg_tol, cg_max_iterations):
    """the engine's linear solve: conjugate gradients from delta = 0, preconditioned by the inverses of the damped diagonal blocks,
    stopped when |res| <= cg_tol |b| or after cg_max_iterations.  -> (delta, iterations)"""
    import scipy.sparse as sp
    n = len(L.fixed)
    free = ~L.fixed
    mask = np.repeat(free, 6).astype(np.float64)
    A = (system_matrix(L) + lam * sp.diags(mask)).tocsr()
    Minv = np.zeros((n, 6, 6))
    if free.any():
        Minv[free] = np.linalg.inv(L.diag[free] + lam * np.eye(6))
        Minv[free] = 0.5 * (Minv[free] + np.swapaxes(Minv[free], 1, 2))
    P = sp.bsr_matrix((Minv, np.arange(n), np.arange(n + 1)), shape=(6 * n, 6 * n)).tocsr()

    def mv(v):
        return A @ v
    x = np.zeros(6 * n)
    r = -L.grad.ravel() * mask
    bnorm2 = float(r @ r)
    if not bnorm2 > 0.0:
        return x.reshape(-1, 6), 0
    z = P @ r
    p = z.copy()
    rz = float(r @ z)
    it = 0
    for it in range(1, cg_max_iterations + 1):
        q = mv(p)
        pq = float(p @ q)
        if not pq > 0.0:
            it -= 1
            break
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        z = P @ r
        rz_new, rr = float(r @ z), float(r @ r)
        if rr <= cg_tol * cg_tol * bnorm2:
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x.reshape(-1, 6), it


def step_sizes(delta, fixed):
    """-> (largest |so3_exp(d_w) - I| entry, largest |d_t| entry) over the free nodes: is_converged's two quantities"""
    if not (~fixed).any():
        return 0.0, 0.0
    d = delta[~fixed]
    return float(np.abs(so3_exp(d[:, :3]) - np.eye(3)).max()), float(np.abs(d[:, 3:]).max())


def optimize(g, solver="direct", **opt):
    """Levenberg-Marquardt on the whole graph with csrc/ngicp_lm.h's schedule.  g.poses is updated in place with the last accepted
    poses.  -> dict(initial_chi2, final_chi2, iterations, accepted, cg_iterations, converged, trace[(chi2 of the try, lambda, rho,
    cg iterations, accepted)], margins[(|rho|, step sizes)])"""
    o = dict(DEFAULTS)
    o.update(opt)
    if ungauged_components(g.n, g.ij, g.fixed):
        raise Refused("a connected component holds no fixed node")
    L = linearize(g)
    res = dict(initial_chi2=L.chi2, final_chi2=L.chi2, iterations=0, accepted=0, cg_iterations=0, converged=False, trace=[], steps=[])
    free = ~g.fixed
    lam = LM_INIT_LAMBDA_FACTOR * (float(np.abs(np.einsum("nii->ni", L.diag[free])).max()) if free.any() and g.m else 0.0)
    done = False
    while not done and res["iterations"] < o["max_iterations"]:
        nu = 2.0
        res["iterations"] += 1
        for trial in range(LM_MAX_TRIES):
            if solver == "direct":
                delta, its = solve_direct(L, lam)
            else:
                delta, its = solve_pcg(L, lam, o["cg_tol"], o["cg_max_iterations"])
            trial_poses = g.poses.copy()
            trial_poses[free] = left_update(delta[free], g.poses[free])
            Lt = linearize(g, trial_poses)
            den = float(np.sum(delta * (lam * delta - L.grad)))
            with np.errstate(divide="ignore", invalid="ignore"):
                rho = np.float64(L.chi2 - Lt.chi2) / np.float64(den)
            rot, trans = step_sizes(delta, g.fixed)
            small = max(rot / o["rot_eps"], trans / o["trans_eps"]) < 1
            rejected = bool(rho < 0)  # NaN is accepted, as in the aligner
            res["cg_iterations"] += its
            res["trace"].append((Lt.chi2, lam, float(rho), its, 0 if rejected else 1))
            res["steps"].append((rot, trans))
            if rejected:
                if small:
                    res["converged"], done = True, True
                    break
                lam, nu = nu * lam, 2 * nu
                if trial + 1 >= LM_MAX_TRIES:
                    done = True
                continue
            g.poses = trial_poses
            L = Lt
            res["accepted"] += 1
            res["final_chi2"] = L.chi2
            q = 2 * rho - 1
            lam = lam * max(1.0 / 3.0, 1 - q * q * q)
            if small:
                res["converged"], done = True, True
            break
    return res


# ---------------------------------------------------------------- corrections, edge_from_alignment
def _mul3(a0, a1, a2, b0, b1, b2):
    return a0 * b0 + a1 * b1 + a2 * b2


def correction(T_new, T_old):
    """C = T_new * T_old^-1 in the engine's order of operations (csrc/ngicp_pose_graph.h, k_pg_corrections), rounded to float32.
    T_old^-1 = (R^T, -(R^T t)) with every sum (a0 b0 + a1 b1) + a2 b2; then pose_mul's products in the same order."""
    Tn, To = np.asarray(T_new, np.float64), np.asarray(T_old, np.float64)
    Ri = To[:3, :3].T.copy()
    ti = np.array([-_mul3(Ri[r, 0], Ri[r, 1], Ri[r, 2], To[0, 3], To[1, 3], To[2, 3]) for r in range(3)])
    C = np.eye(4)
    for r in range(3):
        for c in range(3):
            C[r, c] = _mul3(Tn[r, 0], Tn[r, 1], Tn[r, 2], Ri[0, c], Ri[1, c], Ri[2, c])
        C[r, 3] = _mul3(Tn[r, 0], Tn[r, 1], Tn[r, 2], ti[0], ti[1], ti[2]) + Tn[r, 3]
    return C.astype(np.float32)


def corrections(T_new, T_old):
    return np.stack([correction(a, b) for a, b in zip(T_new, T_old)])


def edge_from_alignment(T_i, T_aligned, H):
    """-> (Z, Lambda): Z = T_i^-1 T_aligned, and H (the aligner's information, in its left perturbation of the world pose T_aligned)
    expressed in the edge's residual coordinates: r = J d at the measurement, J = [[A, 0], [-A [t]x, A]] with A = R_aligned^T and
    t = t_aligned, so Lambda = J^-T H J^-1 with J^-1 = [[A^T, 0], [[t]x A^T, A^T]]; symmetrised exactly."""
    T_i, T_a, H = np.asarray(T_i, np.float64), np.asarray(T_aligned, np.float64), np.asarray(H, np.float64)
    Z = inv_pose(T_i) @ T_a
    At = T_a[:3, :3]
    Jinv = np.zeros((6, 6))
    Jinv[:3, :3] = At
    Jinv[3:, :3] = skew(T_a[:3, 3]) @ At
    Jinv[3:, 3:] = At
    Lam = Jinv.T @ H @ Jinv
    return Z, 0.5 * (Lam + Lam.T)
