"""The optimiser's step in its two forms: lm_step on one lane (NGICP_SERIAL_STEP=1, the reference form) and lm_step_wave on a whole wave
(the default) must agree bit for bit (-m gpu).

Part 1 runs single steps through ngicp_step_selftest (both forms from the same state image, sums and configuration) and compares the
two resulting records byte by byte: the state image, the trace row, d and the flags.  Where a trial was made and the system is well
conditioned (cond_2 <= 1e3: the forward error of an LDL^T solve and of numpy's LU, ~ n * eps * cond each, stays below 1e-11), d also
agrees with numpy.linalg.solve in float64 to 1e-10 relative.

Part 2 runs whole alignments on two small shapes in fresh child processes (tests/_solver_step_worker.py), once with NGICP_SERIAL_STEP=1
and once without, under the default route, NGICP_FUSED=1 and NGICP_PERSIST=1, and compares everything the alignment reports except times (the robust kernel under the default route only: the other two have no
robust build of the pass)."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_solver_step_worker.py")

N_IN = 132
# the state image begins with these doubles, in the order of the selftest's input (include/ngicp.h)
X0, XI, DELTA, HH, BB, Y0, DD, LAMBDA, NU = slice(0, 12), slice(12, 24), slice(24, 36), slice(36, 72), slice(72, 78), 78, slice(79, 85), 85, 86
ITER, TRIAL, HAVE_LIN, CUR, N_TRACE, LIN_UNNEEDED = 87, 88, 89, 90, 91, 92
MAX_IT, LM_MAX, OPTIMIZER, ROT_EPS, TRANS_EPS, FACTOR = 93, 94, 95, 96, 97, 98
SUMS, SEARCHED = slice(99, 131), 131
IU = np.triu_indices(6)  # row-major upper triangle: the order of tri21


def _rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _pose(rng, rot=0.3, trans=2.0):
    return np.concatenate([_rot(rng.normal(size=3) * rot).ravel(), rng.normal(size=3) * trans])


def _row(rng, A, b, path, *, lam=None, d=None, delta=None, it=3, trial=0, max_it=32, lm_max=10, n_trace=0, yi=None, eps=(2e-3, 0.01), factor=1e-9):
    """One problem.  A, b: the system the step's trial solves (placed in the state AND in the sums, so that every path - first pass,
    accepted, rejected, Gauss-Newton - factorises it; lambda is added by the path).  path: first | accept | reject | gn."""
    r = np.zeros(N_IN)
    r[X0], r[XI] = _pose(rng), _pose(rng)
    r[DELTA] = _pose(rng, 0.05, 0.2) if delta is None else delta
    r[HH], r[BB] = np.asarray(A, float).ravel(), b
    r[Y0] = 1e3 * (1 + rng.random())
    r[DD] = rng.normal(size=6) * 1e-2 if d is None else d
    r[LAMBDA] = (10.0 ** rng.uniform(-6, 3)) if lam is None else lam
    r[NU] = 2.0 ** rng.integers(1, 5)
    r[ITER], r[TRIAL], r[HAVE_LIN], r[CUR], r[N_TRACE] = it, trial, 0 if path == "first" else 1, rng.integers(0, 2), n_trace
    r[MAX_IT], r[LM_MAX], r[OPTIMIZER], r[ROT_EPS], r[TRANS_EPS], r[FACTOR] = max_it, lm_max, 0 if path == "gn" else 1, eps[0], eps[1], factor
    s = np.zeros(32)
    s[:21], s[21:27], s[27] = np.asarray(A, float)[IU], b, r[Y0] * (0.5 + rng.random())
    with np.errstate(all="ignore"):
        den = float(np.sum(r[DD] * (r[LAMBDA] * r[DD] - r[BB])))
    rho = {"accept": 0.1 + rng.random(), "reject": -0.1 - rng.random()}.get(path, 0.5)
    s[28] = (r[Y0] - rho * den) if yi is None else yi
    s[29:32] = rng.integers(0, 10**6, 3)
    r[SUMS], r[SEARCHED] = s, rng.integers(0, 2)
    return r


def _spd(rng, lo, hi):
    B = rng.normal(size=(6, 8))
    C = B @ B.T
    C /= np.sqrt(np.outer(np.diag(C), np.diag(C)))
    s = np.sqrt(10.0 ** rng.uniform(lo, hi, 6))
    A = C * np.outer(s, s)
    return (A + A.T) / 2


def _problems():
    rng = np.random.default_rng(20260517)
    paths = ("first", "accept", "reject", "gn")
    rows = []
    add = rows.append
    # random SPD systems over the scale range of a real H, and well-conditioned ones (the numpy comparison), on every path
    for n in range(2400):
        A = _spd(rng, 2, 9) if n % 3 else _spd(rng, 3, 4)
        add(_row(rng, A, rng.normal(size=6) * np.sqrt(np.diag(A)), paths[n % 4], lam=(-1.0 if n % 8 == 0 else None)))
    # every pivot permutation: distinct diagonal magnitudes in each of the 720 orders
    for n, perm in enumerate(itertools.permutations(range(6))):
        S = rng.normal(size=(6, 6)) * 20.0
        A = np.diag(1e3 * (np.array(perm) + 1.0)) + (S + S.T) / 2
        add(_row(rng, A, rng.normal(size=6) * 30, paths[n % 4], lam=1e-3))
    # equal diagonal magnitudes (the lowest index wins), also with opposite signs; negative and zero diagonals
    for n in range(300):
        S = rng.normal(size=(6, 6))
        dg = np.full(6, 5.0)
        if n % 3 == 1:
            dg[rng.integers(0, 6, 2)] = 7.0
        if n % 3 == 2:
            dg *= rng.choice([-1.0, 1.0], 6)
        add(_row(rng, np.diag(dg) + 0.3 * (S + S.T), rng.normal(size=6), ("reject", "gn")[n % 2], lam=0.0))
    for n in range(300):
        S = rng.normal(size=(6, 6))
        dg = rng.normal(size=6) * 10
        dg[rng.integers(0, 6, rng.integers(0, 4))] = 0.0
        add(_row(rng, np.diag(dg) + (S + S.T), rng.normal(size=6), ("reject", "gn", "accept", "first")[n % 4], lam=(0.0 if n % 2 else 1e-2)))
    # a zero, infinite or NaN pivot in each position (lambda 0: the skip branch is met exactly)
    for k in range(6):
        for bad in (0.0, np.inf, -np.inf, np.nan):
            for path in ("reject", "gn"):
                dg = np.concatenate([10.0 - np.arange(k), np.zeros(6 - k)])
                A = np.diag(dg)
                if k:
                    S = rng.normal(size=(k, k)) * 0.1
                    A[:k, :k] += S + S.T
                if bad != 0.0:
                    A[k, k] = bad  # (an infinity is chosen first, a NaN at k when the search reaches it)
                add(_row(rng, A, rng.normal(size=6), path, lam=0.0))
    # NaN and Inf in H, b and yi
    for n in range(240):
        A = _spd(rng, 2, 6)
        b = rng.normal(size=6) * 100
        yi = None
        bad = (np.nan, np.inf, -np.inf)[n % 3]
        where = n % 4
        if where == 0:
            i, j = rng.integers(0, 6, 2)
            A[i, j] = A[j, i] = bad
        elif where == 1:
            b[rng.integers(0, 6)] = bad
        elif where == 2:
            yi = bad
        else:
            A[rng.integers(0, 6), rng.integers(0, 6)] = bad  # (one triangle only)
        add(_row(rng, A, b, paths[(n // 4) % 4], yi=yi))
    # rotation vectors on both sides of so3_exp's Taylor switch (|w|^2 < 1e-10), and exactly zero
    for n in range(200):
        A = _spd(rng, 3, 4)
        w = rng.normal(size=3)
        w *= (0.0, 1e-7, 0.999e-5, 1.001e-5, 1e-3)[n % 5] / np.linalg.norm(w)
        dt = np.concatenate([w, rng.normal(size=3) * 1e-3])
        add(_row(rng, A, -A @ dt, ("reject", "gn")[n // 5 % 2], lam=0.0))  # (lambda 0 on both paths: the solve returns ~dt)
    # the state machine's corners
    ident = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    for n in range(400):
        A = _spd(rng, 3, 5)
        b = rng.normal(size=6) * np.sqrt(np.diag(A))
        tiny = rng.normal(size=6) * 1e-9  # a step below the convergence thresholds: lin_unneeded through is_converged
        c = n % 10
        if c == 0: add(_row(rng, A, b, "reject", trial=9, lm_max=10))                       # reject until lm_max_iterations
        elif c == 1: add(_row(rng, A, b, "accept", it=31, max_it=32))                       # accepted in the last outer iteration
        elif c == 2: add(_row(rng, A, b, "accept", it=30, max_it=32))                       # the trial made is the last iteration's
        elif c == 3: add(_row(rng, A, b, "accept", delta=ident + rng.normal(size=12) * 1e-6))   # converged, accepted
        elif c == 4: add(_row(rng, A, b, "reject", delta=ident + rng.normal(size=12) * 1e-6))   # converged, rejected
        elif c == 5: add(_row(rng, A, -A @ tiny, ("accept", "reject", "first")[n // 10 % 3], lam=1e-9))  # the trial made converges
        elif c == 6: add(_row(rng, A, b, "first", lm_max=(0, -1)[n // 10 % 2]))             # lm_max_iterations <= 0
        elif c == 7: add(_row(rng, A, b, "gn", it=(14, 3)[n // 10 % 2], max_it=15))         # Gauss-Newton, last iteration or not
        elif c == 8: add(_row(rng, A, -A @ tiny, "gn"))                                     # Gauss-Newton, converged
        else: add(_row(rng, A, b, ("accept", "reject")[n // 10 % 2], n_trace=1))            # the trace is full
    return np.array(rows)


@pytest.fixture(scope="module")
def steps(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    P = _problems()
    g = nano_gicp.NanoGICP()
    out = g.stepSelftest(P)
    g.close()
    return P, out


def _view(out, form):
    rec = out[:, form, :]
    nimg = rec.shape[1] - 18 * 8
    img = np.ascontiguousarray(rec[:, :87 * 8]).view(np.float64)
    tail = np.ascontiguousarray(rec[:, nimg:]).view(np.float64)
    return img, tail


def test_wave_step_equals_serial_step_byte_for_byte(steps):
    P, out = steps
    diff = np.flatnonzero((out[:, 0, :] != out[:, 1, :]).any(axis=1))
    img, tail = _view(out, 0)
    done, conv, failed = tail[:, 14], tail[:, 15], tail[:, 16]
    lm = P[:, OPTIMIZER] == 1
    print(f"{len(P)} steps; differing {len(diff)}; done {int(done.sum())}, converged {int(conv.sum())}, lm_failed {int(failed.sum())}")
    # the cases meet the branches they were written for
    assert (done[lm] == 0).sum() > 500 and (done[lm] == 1).sum() > 50 and failed.sum() >= 30 and conv.sum() >= 60
    assert ((tail[:, 7] == 1) & lm).any() and ((tail[:, 7] == 0) & (tail[:, 5] != 0) & lm).any()  # accepted and rejected trace rows
    assert len(diff) == 0, f"steps {diff[:20].tolist()} differ; first: fields (8-byte words) {np.flatnonzero((out[diff[0], 0] != out[diff[0], 1]).reshape(-1, 8).any(axis=1)).tolist()}"


def test_solved_step_agrees_with_numpy(steps):
    P, out = steps
    img, tail = _view(out, 1)
    checked, worst = 0, 0.0
    for n in range(len(P)):
        gn = P[n, OPTIMIZER] == 0
        if not gn and tail[n, 14] != 0:
            continue  # the alignment ended without another trial
        A = img[n, HH].reshape(6, 6) + (0.0 if gn else img[n, LAMBDA]) * np.eye(6)
        b = img[n, BB]
        if not (np.isfinite(A).all() and np.isfinite(b).all() and np.array_equal(A, A.T)) or np.linalg.cond(A) > 1e3:
            continue
        ref = np.linalg.solve(A, -b)
        err = np.abs(tail[n, 8:14] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        checked += 1
        assert err <= 1e-10, f"step {n}: d differs from numpy by {err:.3e} relative"
    print(f"{checked} well-conditioned systems compared with numpy, worst relative difference {worst:.3e}")
    assert checked > 200


# ---- part 2: whole alignments, NGICP_SERIAL_STEP=1 against the default, per route ----
ROUTES = {"default": {}, "fused": {"NGICP_FUSED": "1"}, "persist": {"NGICP_PERSIST": "1"}}
SWITCHES = ("NGICP_SERIAL_STEP", "NGICP_FUSED", "NGICP_PERSIST", "NGICP_HEAD", "NGICP_QUEUE", "NGICP_PASS_IMPL")


@pytest.mark.parametrize("route", list(ROUTES))
def test_alignments_equal_under_serial_and_wave_step(hip_lib, route):
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    base.update(ROUTES[route])
    children = [subprocess.Popen([sys.executable, WORKER], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                                 env=dict(base, **extra)) for extra in ({"NGICP_SERIAL_STEP": "1"}, {})]
    results = []
    for child in children:
        try:
            so, se = child.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for c in children:
                c.kill()
            pytest.fail(f"{route}: a child gave no result in 240 s")
        assert child.returncode == 0, f"{route}: exit {child.returncode}\n{so[-2000:]}\n{se[-4000:]}"
        results.append(json.loads([l for l in so.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]))
    serial, wave = results
    assert serial["serial_step"] == "1" and wave["serial_step"] == ""
    assert sorted(serial["scenarios"]) == sorted(wave["scenarios"]) and len(serial["scenarios"]) == (16 if route == "default" else 14)
    rejected = {n: [r[2] == 0 for r in s["trace_rows"]] for n, s in serial["scenarios"].items()}
    print(route, {n: (s["passes"], s["iters"], sum(rejected[n]), s.get("groups")) for n, s in serial["scenarios"].items()})  # (passes, iterations, rejected trials, groups)
    for name, s in serial["scenarios"].items():
        assert s == wave["scenarios"][name], f"{route}/{name}: " + ", ".join(k for k in s if s[k] != wave["scenarios"][name][k])
        assert s["passes"] >= 1
    assert any(rejected["30k_30k/far_guess"]), "no trial was rejected from the far guess"
    assert any(rejected["10k_10k/rejections"][:-1]), "no rejected trial was followed by another trial"
    assert rejected["10k_10k/rejections_lm_max2"][-1], "lm_max_iterations = 2 did not end the alignment on a rejected trial"
    assert serial["scenarios"]["2k_5k/dlo"]["groups"] < 32 and 100 <= serial["scenarios"]["30k_30k/dlo"]["groups"] <= 1000
