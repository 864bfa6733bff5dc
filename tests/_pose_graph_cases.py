"""Pose-graph fixtures shared by tests/test_pose_graph_model_cpu.py and tests/test_gpu_pose_graph.py.   *** TEST INFRASTRUCTURE ONLY ***

Every case is (graph at its drifted start, ground-truth poses).  Truth is a seeded random walk; a measurement is the truth's relative
pose, times a small seeded noise pose unless noise-free; the start is the truth's chain re-integrated in node order with a drift of up
to 3 degrees and 0.5 m per node (scaled by sqrt(256 / n) on longer graphs, so that no edge's residual rotation comes near so3_log's
3 rad).  Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

import _pose_graph_model as pgm

SIGMA_ROT, SIGMA_TRANS = 0.005, 0.02
# The options every optimiser comparison runs with.  The epsilons: Levenberg-Marquardt gains a factor of about a hundred per step near the
# end, so the last step tried is 1e-6 or more and lowers chi2 by 1e-9 or more - far above the rounding of chi2 itself (1e-14), so that
# the gain ratio of the last try is not noise.  cg_tol is the engine's default (but see big4097 below).
OPTIONS = dict(max_iterations=40, rot_eps=1e-4, trans_eps=1e-4, cg_tol=1e-8, cg_max_iterations=30000)
# big4097 stops after two outer iterations: its conjugate gradients need 13 000 to 19 000 iterations per solve (a chain bends like a beam),
# and the model's run to convergence (8 tries) takes 80 s in numpy.  Two tries still cover accept, re-linearise and the iteration cap.
# Its cg_tol is 1e-11: after two iterations the poses are not at a minimum, so chi2 responds in FIRST order to what the truncated solve
# leaves out - at the default 1e-8 the model's own two solvers already differ by 3e-7 of chi2 there (and by 8.4e-6 in the poses), which the
# 1e-9 comparison of chi2 cannot pass whatever the engine does; at 1e-11 they differ by 3e-12 of chi2 and 5.6e-9 in the poses.
CASE_OPTIONS = {"big4097": dict(max_iterations=2, cg_tol=1e-11)}


def options(name):
    o = dict(OPTIONS)
    o.update(CASE_OPTIONS.get(name, {}))
    return o


def _rand_pose(rng, rot, trans):
    return pgm.make_pose(rng.uniform(-rot, rot, 3), rng.uniform(-trans, trans, 3))


def truth_walk(n, seed):
    rng = np.random.default_rng(seed)
    T = [pgm.make_pose(rng.uniform(-0.3, 0.3, 3), rng.uniform(-5, 5, 3))]
    for _ in range(n - 1):
        T.append(T[-1] @ pgm.make_pose(rng.uniform(-0.25, 0.25, 3), np.r_[rng.uniform(0.5, 2.0), rng.uniform(-0.3, 0.3, 2)]))
    return np.stack(T)


def drifted(truth, seed, scale=1.0):
    rng = np.random.default_rng(seed + 1000)
    n = len(truth)
    k = scale * min(1.0, np.sqrt(256.0 / n))
    S = [truth[0].copy()]
    for a in range(1, n):
        S.append(S[-1] @ (pgm.inv_pose(truth[a - 1]) @ truth[a]) @ _rand_pose(rng, k * np.deg2rad(3.0), k * 0.5))
    return np.stack(S)


def information(rng):
    """a full symmetric positive-definite 6x6: diag(1 / sigma^2) in a slightly rotated basis, mirrored entries exactly equal"""
    A = rng.normal(size=(6, 6)) * 0.05
    Q = np.linalg.qr(np.eye(6) + A - A.T)[0]
    d = np.r_[np.full(3, 1.0 / SIGMA_ROT ** 2), np.full(3, 1.0 / SIGMA_TRANS ** 2)] * rng.uniform(0.5, 2.0, 6)
    L = Q @ np.diag(d) @ Q.T
    return 0.5 * (L + L.T)


def build(truth, pairs, fixed_ids, seed, noisy=True, flags=None, drift_scale=1.0, noise_scale=1.0):
    rng = np.random.default_rng(seed + 2000)
    g = pgm.Graph()
    fixed = np.zeros(len(truth), bool)
    fixed[list(fixed_ids)] = True
    g.add_nodes(drifted(truth, seed, drift_scale), fixed)
    Z, info = [], []
    for a, b in pairs:
        z = pgm.inv_pose(truth[a]) @ truth[b]
        if noisy:
            z = z @ pgm.make_pose(rng.normal(0, noise_scale * SIGMA_ROT, 3), rng.normal(0, noise_scale * SIGMA_TRANS, 3))
        Z.append(z)
        info.append(information(rng))
    Z = np.stack(Z)
    Z[:, 3] = [0.0, 0.0, 0.0, 1.0]
    g.add_edges(np.array(pairs), Z, np.stack(info), flags)
    return g, truth


def chain_pairs(n):
    return [(a, a + 1) for a in range(n - 1)]


def pair(seed=11):
    return build(truth_walk(2, seed), [(0, 1)], [0], seed)


def three_mid_fixed(seed=12):
    return build(truth_walk(3, seed), chain_pairs(3), [1], seed)


def chain(n, seed=13):
    return build(truth_walk(n, seed + n), chain_pairs(n), [0], seed + n)


def ring24(seed=14, noisy=True, false_edge=False):
    """a chain of 24 with one loop edge 23 -> 0; false_edge: plus a FLAGGED false loop edge joining opposite sides (6 -> 18), the true
    loop edge flagged too (odometry unflagged)"""
    truth = truth_walk(24, seed)
    pairs = chain_pairs(24) + [(23, 0)]
    flags = None
    if false_edge:
        pairs = pairs + [(6, 18)]
        flags = np.r_[np.zeros(23, bool), True, True]
    g, truth = build(truth, pairs, [0], seed, noisy, flags)
    if false_edge:
        rng = np.random.default_rng(seed + 3000)
        g.Z[-1] = _rand_pose(rng, 0.4, 3.0)  # nothing to do with T_6^-1 T_18
    return g, truth


def star130(seed=15):
    """hub 0 with 130 edges (alternately given as (hub, leaf) and (leaf, hub)); leaf 1 is the fixed node; five leaf-leaf edges"""
    truth = truth_walk(131, seed)
    pairs = [(0, a) if a % 2 else (a, 0) for a in range(1, 131)] + [(5, 90), (17, 3), (44, 45), (130, 2), (64, 65)]
    return build(truth, pairs, [1], seed, drift_scale=0.3)


def multi_edge(seed=16):
    """three edges between 0 and 1, one of them as (1, 0); (3, 2) given with j < i"""
    return build(truth_walk(4, seed), [(0, 1), (0, 1), (1, 0), (1, 2), (3, 2), (0, 3)], [0], seed)


def two_components(seed=17):
    truth = truth_walk(11, seed)
    pairs = chain_pairs(6) + [(5, 0)] + [(a, a + 1) for a in range(6, 10)] + [(10, 6)]
    return build(truth, pairs, [2, 9], seed)


def laps(n, seed, radius=15.0, step=0.5):
    """a platform driving laps on a circle, heading along the tangent, with a little wobble: n poses that stay near the origin"""
    rng = np.random.default_rng(seed)
    T = []
    for k in range(n):
        a = k * step / radius
        T.append(pgm.make_pose(np.r_[rng.normal(0, 0.02, 2), a + np.pi / 2 + rng.normal(0, 0.02)],
                               np.r_[radius * np.cos(a), radius * np.sin(a), 0.0] + rng.normal(0, 0.05, 3)))
    return np.stack(T)


def big(seed=18, n=4097, loops=40, drift_scale=0.3, noise_scale=0.3):
    """a chain of 4097 with 40 random loop edges (either direction).  The trajectory laps a 15 m circle: Levenberg-Marquardt then needs
    8 tries from the drifted start, where a 400 m random walk needs 19 and more (measured on the model)"""
    truth = laps(n, seed)
    rng = np.random.default_rng(seed + 4000)
    pairs = chain_pairs(n)
    for _ in range(loops):
        a, b = sorted(rng.choice(n, 2, replace=False))
        pairs.append((int(b), int(a)) if rng.random() < 0.5 else (int(a), int(b)))
    return build(truth, pairs, [0], seed, drift_scale=drift_scale, noise_scale=noise_scale)


ROBUST_WIDTH = 3.0  # the false-loop-edge fixtures' kernel width: three sigma in the residual's whitened units


def false_edge(kind):
    """ring24 plus one flagged false loop edge, under the robust kernel `kind` (NONE: the false edge pulls with its full weight)"""
    g, truth = ring24(false_edge=True)
    g.kind, g.width = kind, ROBUST_WIDTH
    return g, truth


CASES = {
    "false_edge_none": lambda: false_edge(pgm.NONE), "false_edge_cauchy": lambda: false_edge(pgm.CAUCHY),
    "pair": pair, "three_mid_fixed": three_mid_fixed, "chain65": lambda: chain(65), "chain257": lambda: chain(257), "ring24": ring24,
    "star130": star130, "multi_edge": multi_edge, "two_components": two_components, "big4097": big,
}


def pose_difference(A, B):
    """largest entry-wise difference between two pose arrays (rotation entries and translations alike)"""
    return float(np.abs(np.asarray(A)[:, :3, :] - np.asarray(B)[:, :3, :]).max())


# The largest pose difference between the model with its direct solve and the model with its own conjugate gradients at cg_tol = 1e-8
# (tests/test_pose_graph_model_cpu.py measures it and holds these records to what it measures): over every fixture but big4097 (the
# largest is false_edge_none, which is still creeping when the iteration cap ends it), and for big4097, stopped after two outer
# iterations at cg_tol = 1e-11.  Ten times the record is the tolerance of the GPU comparison.
MEASURED_CG_DIFF = {"default": 3e-12, "big4097": 7e-9}


def assert_margins(res, opt):
    """On the model alone: every gain ratio of the trace is further than 1e-6 from the acceptance threshold 0, and no step is within one
    per cent of the stopping thresholds - rounding cannot flip an accept or the stop."""
    for (chi2, lam, rho, its, acc), (rot, trans) in zip(res["trace"], res["steps"]):
        assert abs(rho) > 1e-6, res["trace"]
        q = max(rot / opt["rot_eps"], trans / opt["trans_eps"])
        assert q < 0.99 or q > 1.01, (rot, trans)
