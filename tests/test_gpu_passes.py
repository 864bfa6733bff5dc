"""Every pass of an alignment against the oracle (-m gpu), not only its two ends.

Passes 2..N run code that the cold linearize() hook never runs: the warm start from the previous correspondence, the rows listed for
batches that went far in the pass before, the measured-cost launch order (rebuilt during the alignment and carried over to the next one
on the same handle), the tpt / mahal ping-pong and K4's error on the previous correspondences.  A wrong neighbour for a few queries of a
late pass moves the final pose by far less than any pose tolerance, so each pass is observed on its own, through the public API only:

  * align(guess) with setMaximumIterations(m) runs exactly the first m outer iterations of the longer alignment (the optimiser never
    looks ahead).  Its float pose P_m = pose_to_colmajor_f(x0) is the pose the next pass searches with (xi_f = (float)x0); P_0 = guess.
  * correspondences() after it are those of the last ADOPTED linearisation, the one at P_{m-1} (the reference's correspondences_ after
    align(): its last linearize(), impl/lsq_registration_impl.hpp:162).
  * getFinalHessian() is the H of the last ACCEPTED step (final_hessian_, :155,203): at P_{m-1} too, except when the alignment ended on
    rejected trials (LM gave up, or a rejected step was already below the epsilons) - x0 then stayed where it was, and the H is that of
    the iteration before.

Pass m is compared with a COLD oracle search at the GPU's own pose, OracleGICP.linearize(P_{m-1}), on the same shared covariances: the
same gate decisions, float32 squared distances bit for bit on every gated-in query (and equal to the distance to the returned index,
recomputed here in float32 in the kernel's order), indices equal except on exact float32 distance ties, and H within 1e-5 relative.  The
LM trace's errors of that iteration are compared too: y0 (the linearisation's own error) with the oracle's linearize(P_{m-1}) error, and
the accepted trial's yi (K4: the trial pose under the previous correspondences and Mahalanobis matrices) with the oracle's
compute_error(P_m) after that linearize, both within 1e-5 relative.  These tolerances cover ONLY the float rounding of the pose: the GPU
evaluates at the double pose, the oracle at double(float(pose)) (observed: |dH|/|H| < 1e-7, y0 / yi < 3e-6).  The exact correspondence
check carries the strictness; the H and error checks are there for a dropped or duplicated batch or a stale Mahalanobis buffer, each of
order 1e-4 or more on the passes where the pose still moves.  (Comparing with the oracle's OWN alignment would not work for late passes: the two drift apart by rounding - the
reason the FIXED20 trace checks elsewhere stop at row 4.)

Besides, the trace of align(max_iter=m) must be the first rows of the full run's, bit for bit, and its pose must equal what a fresh
handle's align(max_iter=m) returns - the launch order a reused handle carries over changes nothing."""
import numpy as np
import pytest

from direct_lidar_odometry_amd import clouds

from _pass_check import CASES, DLO, FIXED20, Rig, _configure, _scan_to_scan_rig, _shape, check_passes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


# ------------------------------------------------------------------ 10k scan-to-scan
@pytest.mark.parametrize("case", list(CASES))
def test_every_pass_scan_to_scan_10k(ng, oracle_mod, case):
    rig, guess = _scan_to_scan_rig(ng, oracle_mod, case)
    rig.run(guess, case)
    print(f"{case}: {int((rig.g.lm_trace()[:, 7] == 0).sum())} rejected trials")


@pytest.mark.parametrize("switch", [("NGICP_PERSIST", "1"), ("NGICP_HEAD", "1"), ("NGICP_CELL_BOXES", "1"), ("NGICP_CHUNK", "64")], ids=lambda s: s[0])
@pytest.mark.parametrize("case", list(CASES) + ["c3_fixed20"])
def test_every_pass_under_switches(ng, oracle_mod, monkeypatch, case, switch):
    """The same per-pass checks with each per-handle switch (read at ngicp_create).  NGICP_CHUNK=64 keeps 64 (pass, solve) pairs in
    flight: that many stale ones are still on the stream when align() sees `done` and returns."""
    monkeypatch.setenv(*switch)
    if case == "c3_fixed20":
        w = clouds.scan_to_submap(100_000, 5)
        rig, guess = Rig(ng, oracle_mod, w.source, w.target, 20, w.max_corr_dist, FIXED20, w.keyframe_sizes), w.guess
    else:
        rig, guess = _scan_to_scan_rig(ng, oracle_mod, case)
    rig.run(guess, f"{case} {switch[0]}={switch[1]}")


# ------------------------------------------------------------------ adversarial target shapes, small voxel
@pytest.mark.parametrize("shape", ["cube", "plane", "lines", "clumps"])
def test_every_pass_adversarial_shapes(ng, oracle_mod, shape):
    """Uniform volume, one dense plane, dense lines, tight clumps, aligned from ~0.3 m / 5 deg off with a 0.1 m voxel: a step crosses
    several cells, so the warm start lies cells away from the new neighbour and listed rows change between passes.  The covariances
    are fixed (isotropic): the search is what is under test, and clouds this degenerate would leave the optimiser to rounding."""
    src, tgt = _shape(shape)
    c = np.diag([0.01, 0.01, 0.01, 0.0])
    covs = (np.repeat(c[None], len(src), 0), np.repeat(c[None], len(tgt), 0))
    rig = Rig(ng, oracle_mod, src, tgt, 20, 1.0, dict(setMaximumIterations=12, setTransformationEpsilon=1e-6, setRotationEpsilon=1e-6),
              covs=covs, tuning=0.1)
    assert rig.g.stats()["voxel_size"] <= 0.1 + 1e-9
    rig.run(clouds.make_pose((0.2, -0.15, 0.15), (2.0, -2.0, 4.0)), shape)


# ------------------------------------------------------------------ full size
def _full(ng, orc, w, k, gate, settings, guess, tgt_sizes, label):
    rig = Rig(ng, orc, w.source, w.target, k, gate, settings, tgt_sizes)
    out = rig.run(guess, label)
    print(f"{label}: ties per pass {[t[0] for t in out]}")
    return out


@pytest.mark.parametrize("gate", [1.0, None])
def test_every_pass_c2_100k(ng, oracle_mod, gate):
    w = clouds.scan_to_scan(100_000)
    _full(ng, oracle_mod, w, 10 if gate else 20, gate, DLO if gate else {}, w.guess, None, f"c2 gate {gate}")


@pytest.mark.parametrize("settings", [DLO, FIXED20], ids=["dlo", "fixed20"])
def test_every_pass_c3_100k_500k(ng, oracle_mod, settings):
    w = clouds.scan_to_submap(100_000, 5)
    _full(ng, oracle_mod, w, 20, w.max_corr_dist, settings, w.guess, w.keyframe_sizes, "c3 " + ("fixed20" if settings is FIXED20 else "dlo"))


@pytest.mark.parametrize("settings", [DLO, FIXED20], ids=["dlo", "fixed20"])
def test_every_pass_c5_250k_2m(ng, oracle_mod, settings):
    w = clouds.scan_to_submap(250_000, 8, shape="os1")
    _full(ng, oracle_mod, w, 20, w.max_corr_dist, settings, w.guess, w.keyframe_sizes, "c5 " + ("fixed20" if settings is FIXED20 else "dlo"))


def test_every_pass_500k_source(ng, oracle_mod):
    from types import SimpleNamespace
    w = clouds.scan_to_submap(100_000, 5)
    inv = np.linalg.inv(np.asarray(w.guess, np.float64)).astype(np.float32)
    _full(ng, oracle_mod, SimpleNamespace(source=w.target, target=w.source), 10, 1.0, DLO, inv, None, "500k source")


@pytest.mark.parametrize("g_rank", [1, 4])
def test_every_pass_c4_ranks(ng, oracle_mod, g_rank):
    w = clouds.scan_to_submap(100_000, 5, seed_offset=1000 * g_rank)
    _full(ng, oracle_mod, w, 20, w.max_corr_dist, FIXED20, w.guess, w.keyframe_sizes, f"c4 rank {g_rank}")


# ------------------------------------------------------------------ sequences on one handle
def test_every_pass_sequences_on_one_handle(ng, oracle_mod):
    """What one alignment leaves on a handle (tpt entries, the launch order, the grid buffers, the listed-rows flags) must not leak into
    the next: two guesses, then a smaller target, a swap of source and target, and the same source set again (covariances kept)."""
    w = clouds.scan_to_scan(10_000)
    rig = Rig(ng, oracle_mod, w.source, w.target, 20, 1.0, DLO)
    g, o = rig.g, rig.o
    rig.run(w.guess, "first guess")
    rig.run(clouds.make_pose((0.3, -0.2, 0.05), (1.0, -1.0, 4.0)), "second guess")
    # a smaller target: any index carried over from the larger one would be out of range or wrong
    small = np.ascontiguousarray(w.target[::3])
    ct_small = rig.ct[::3].copy()
    for e in (g, o):
        e.setInputTarget(small)
        e.setTargetCovariances(ct_small)
    check_passes(g, o, w.guess, "smaller target", w.source, small, rig.cs, ct_small, rig.max_iter)
    # swap source and target (covariances travel with the clouds)
    for e in (g, o):
        e.swapSourceAndTarget()
    inv = np.linalg.inv(np.asarray(g.getFinalTransformation(), np.float64)).astype(np.float32)
    check_passes(g, o, inv, "swapped", small, w.source, ct_small, rig.cs, rig.max_iter)
    for e in (g, o):
        e.swapSourceAndTarget()
    # the same source cloud again: same identity, covariances kept
    g.setInputSource(w.source); o.setInputSource(w.source)
    assert g.sourceCovariancesSize() == len(w.source)
    check_passes(g, o, w.guess, "same source again", w.source, small, rig.cs, ct_small, rig.max_iter)


# ------------------------------------------------------------------ constructed gate and tie cases
def _f32_transform(T, p):
    Tf = np.asarray(T, np.float32)
    p = np.asarray(p, np.float32)
    return np.array([((Tf[r, 0] * p[0] + Tf[r, 1] * p[1]) + Tf[r, 2] * p[2]) + Tf[r, 3] for r in range(3)], np.float32)


def _d2(q, t):
    d = (np.asarray(q, np.float32) - np.asarray(t, np.float32)).astype(np.float32)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _place(q, axis, sign, want):
    """A float32 point at float32 squared distance exactly `want` from q (or None): along `axis` (sign), and where the steps of dx^2 are coarser
    than one ulp of d^2 (they are, a few metres from the origin), with the small remainder made up on a second axis."""
    q = np.asarray(q, np.float32)
    x = np.float32(q[axis] + np.float32(sign * np.sqrt(np.float64(want))))
    for _ in range(64):  # from the closest x inwards, so that the remainder is >= 0
        t = q.copy()
        t[axis] = x
        rest = np.float64(want) - np.float64(_d2(q, t))
        for other in ((axis + 1) % 3, (axis + 2) % 3):
            if rest < 0:
                break
            y0 = np.float32(q[other] + np.float32(np.sqrt(rest)))
            for k in range(-64, 65):
                u = t.copy()
                u[other] = np.float32(y0 + np.float32(k) * np.spacing(y0))
                if _d2(q, u) == want:
                    return u
        x = np.float32(x - np.float32(sign) * np.spacing(x))
    return None  # (rare: a few directions have no such point within reach of the search; the caller takes another)


@pytest.mark.parametrize("gate", [0.5, 0.3])
def test_constructed_gate_and_tie_cases(ng, oracle_mod, gate):
    """Isolated probe queries 12 m above the scan whose only candidates are target points placed so that, at the float pose a given pass
    searches with, the float32 d^2 is one ulp below, equal to (0.5: 0.25 is exact) or nearest to (0.3: 0.09 is not a float), and one ulp
    above the gate^2 (the search prunes at the float bound of gate^2, the gate itself compares in double).  Pass 1 (the guess) also has
    exact duplicates (a tie at every pose, so in every warm pass too) and pairs exactly equidistant from their query.  Passes 2 and 3 get
    boundary probes of their own, built at the GPU's P_1 / P_2 on the side away from where the query was before: still gated out in the
    earlier passes, so that adding them does not move the poses they were built for (checked)."""
    w = clouds.scan_to_scan(10_000)
    rng = np.random.default_rng(7)
    g2 = np.float64(gate) * np.float64(gate)
    near = np.float32(g2)
    below = near if np.float64(near) < g2 else np.nextafter(near, np.float32(0), dtype=np.float32)
    above = near if np.float64(near) > g2 else np.nextafter(near, np.float32(1), dtype=np.float32)
    wants = [below, near, above]
    # group 0: 3 boundary + 3 duplicate + 3 equidistant probes; groups 1 and 2: 3 boundary probes each; all 4 m apart
    probes = [np.array([[dx, dy, 12.0 + 3.0 * grp] for dx in (-4.0, 0.0, 4.0) for dy in (-4.0, 0.0, 4.0)][:9 if grp == 0 else 3], np.float32)
              + rng.uniform(-0.2, 0.2, (9 if grp == 0 else 3, 3)).astype(np.float32) for grp in range(3)]
    src = np.ascontiguousarray(np.concatenate([w.source] + probes))
    n0 = len(w.source)
    c_probe = np.diag([0.01, 0.01, 0.01, 0.0])
    cs = np.concatenate([oracle_mod.covariances(w.source, 20), np.repeat(c_probe[None], len(src) - n0, 0)])
    ct0 = oracle_mod.covariances(w.target, 20)
    settings = dict(setMaximumIterations=6, setTransformationEpsilon=1e-12, setRotationEpsilon=1e-12)
    guess = w.guess
    extra, built = [], []  # probe target points; (group, query row, target row, wanted d2)
    poses = [np.asarray(guess, np.float32)]

    def gpu_poses(tgt, ct, n):
        g = ng.NanoGICP()
        _configure(g, 20, gate, settings)
        g.setInputSource(src); g.setInputTarget(tgt); g.setSourceCovariances(cs); g.setTargetCovariances(ct)
        out = []
        for m in range(1, n + 1):
            g.setMaximumIterations(m)
            g.align(guess)
            out.append(g.getFinalTransformation().copy())
        g.close()
        return out

    for grp in range(3):
        T = poses[grp]
        for j, p in enumerate(probes[grp]):
            q = _f32_transform(T, p)
            before = [_f32_transform(P, p) for P in poses[:grp]]
            if j < 3:  # the gate boundary: of the six axis directions, the one farthest from the query's earlier positions
                best = None
                for axis in range(3):
                    for sign in (1.0, -1.0):
                        t = _place(q, axis, sign, wants[j])
                        if t is None:
                            continue
                        margin = min([_d2(b, t) for b in before], default=np.float32(np.inf))
                        if best is None or margin > best[0]:
                            best = (margin, t)
                assert best is not None and best[0] > g2 * (1 + 1e-5), f"group {grp}: the query has not moved far enough to place its probe ({best[0]!r})"
                built.append((grp, n0 + sum(len(x) for x in probes[:grp]) + j, len(extra), wants[j]))
                extra.append(best[1])
            elif j < 6:  # an exact duplicate pair, well inside the gate
                t = q.copy(); t[j - 3] = np.float32(t[j - 3] + np.float32(0.5 * gate))
                extra += [t, t.copy()]
            else:  # two points exactly equidistant from the query, on both sides of it along one axis
                a = j - 6
                t1, t2 = q.copy(), q.copy()
                t1[a] = np.float32(q[a] + np.float32(0.25 * gate))
                t2[a] = np.float32(q[a] - np.float32(t1[a] - q[a]))
                assert _d2(q, t1) == _d2(q, t2)
                extra += [t1, t2]
        tgt = np.ascontiguousarray(np.concatenate([w.target, np.array(extra, np.float32)]))
        ct = np.concatenate([ct0, np.repeat(c_probe[None], len(extra), 0)])
        poses = [poses[0]] + gpu_poses(tgt, ct, grp + 1)
    # the probes added for a later pass left the earlier poses where they were built
    assert all(np.array_equal(a, b) for a, b in zip(poses[1:], gpu_poses(tgt, ct, 3)))
    rig = Rig(ng, oracle_mod, src, tgt, 20, gate, settings, covs=(cs, ct))
    out = rig.run(guess, f"constructed gate {gate}")
    assert len(out) >= 3
    # each boundary probe sits where it was built in the pass it was built for, and the gate decides on the double gate^2
    o = rig.o
    for grp, row, trow, want in built:
        o.linearize(np.asarray(poses[grp], np.float64))
        co, so = o.correspondences()
        assert so[row] == want, (grp, row, so[row], want)
        assert (co[row] >= 0) == (np.float64(want) < g2), (grp, row, co[row], want)
        assert co[row] in (-1, len(w.target) + trow)
    print(f"gate {gate}: boundary d2 {sorted({float(x) for x in wants})}, ties per pass {[t[0] for t in out]}")
