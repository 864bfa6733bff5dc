"""What the registration loop leaves in stats() and on the handle besides the pose (-m gpu): the profiling counts of every route, the
max_iter = 0 shortcut of the four alignment entries, and what a voxelized align must leave alone for the exact one after it.

The per-pass oracle checks (test_gpu_passes.py and the modules that share _pass_check.py) pin the poses, traces and correspondences of
every route; these tests pin the bookkeeping around them.  All of them run on the 10k dlo_s2s rig of _pass_check.py.  The expected values
are what the code says: with HIP events, launch i of an alignment is timed when i % stride == stride // 2, and the times are summed over
the launches below `passes`; the persistent kernel stamps its own passes instead."""
import math

import numpy as np
import pytest

from _pass_check import _scan_to_scan_rig, handle_env

pytestmark = pytest.mark.gpu

VOXEL_RES = 1.0


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture(scope="module")
def rig_guess(ng, oracle_mod):
    return _scan_to_scan_rig(ng, oracle_mod, "dlo_s2s")


def _handle(rig, env=None, voxel=False):
    with handle_env(env):
        g = rig.handle()
    g.setMaximumIterations(rig.max_iter)
    if voxel:
        g.setVoxelResolution(VOXEL_RES)  # (DIRECT1 is the default neighbourhood)
    return g


def _align(g, guess):
    g.align(guess)
    return dict(T=g.getFinalTransformation().copy(), H=g.getFinalHessian().copy(), trace=g.lm_trace().copy(), it=g.nr_iterations_,
                conv=g.converged_, stats=g.stats())


def _same(a, b):
    return (np.array_equal(a["T"], b["T"]) and np.array_equal(a["H"], b["H"]) and np.array_equal(a["trace"], b["trace"])
            and (a["it"], a["conv"]) == (b["it"], b["conv"]))


def _check_wait_and_times(s):
    assert s["host_wait_spins"] >= 0
    assert s["align_ms"] >= s["loop_ms"] > 0, (s["align_ms"], s["loop_ms"])


def _profiled_and_plain(rig, guess, env=None, voxel=False):
    plain = _handle(rig, env, voxel)
    off = _align(plain, guess)
    plain.close()
    g = _handle(rig, env, voxel)
    g.setProfiling(1)
    on = _align(g, guess)
    g.close()
    print(f"env {env} voxel {voxel}: passes {on['stats']['passes']}, timed {on['stats']['passes_timed']}, pass_ms_total {on['stats']['pass_ms_total']!r}, "
          f"loop_ms {on['stats']['loop_ms']!r}, align_ms {on['stats']['align_ms']!r}, spins {on['stats']['host_wait_spins']}")
    return off, on


@pytest.mark.parametrize("route", ["default", "voxel_direct1", "head"])
def test_profiling_times_every_pass(rig_guess, route):
    """setProfiling(1): one pair of events per pass launch; the count is over passes (the head route launches one kernel more than it has
    passes), and the alignment itself is what it is with profiling off, bit for bit."""
    rig, guess = rig_guess
    off, on = _profiled_and_plain(rig, guess, {"NGICP_HEAD": "1"} if route == "head" else None, route == "voxel_direct1")
    s = on["stats"]
    assert s["passes"] > 0 and s["passes_timed"] == s["passes"]
    assert math.isfinite(s["pass_ms_total"]) and s["pass_ms_total"] > 0
    assert _same(on, off)
    assert off["stats"]["passes_timed"] == 0 and off["stats"]["pass_ms_total"] == 0
    for r in (on, off):
        _check_wait_and_times(r["stats"])
    if route == "voxel_direct1":
        assert s["staged_fraction"] == 0


def test_profiling_persistent_route(rig_guess):
    """NGICP_PERSIST=1: the pass times come from the kernel's own ticks (a pass whose two stamps do not advance is not counted), and the
    alignment is the default route's bit for bit.  (No skip rule: where the persistent kernel cannot run, the handle takes one launch per
    pass and times it with events, which satisfies the same bounds.)"""
    rig, guess = rig_guess
    plain = _handle(rig)
    ref = _align(plain, guess)
    plain.close()
    off, on = _profiled_and_plain(rig, guess, {"NGICP_PERSIST": "1"})
    s = on["stats"]
    assert s["passes"] > 0 and 0 < s["passes_timed"] <= s["passes"]
    assert math.isfinite(s["pass_ms_total"]) and s["pass_ms_total"] > 0
    assert _same(on, ref) and _same(off, ref)
    for r in (on, off):
        _check_wait_and_times(r["stats"])


def test_profiling_stride_and_switching_off(rig_guess):
    """setProfiling(4) times launches 2, 6, 10, ...; setProfiling(0) afterwards leaves no times behind."""
    rig, guess = rig_guess
    g = _handle(rig)
    g.setProfiling(4)
    r = _align(g, guess)
    s = r["stats"]
    print(f"stride 4: passes {s['passes']}, timed {s['passes_timed']}")
    assert s["passes_timed"] == len(range(2, s["passes"], 4))
    g.setProfiling(0)
    r0 = _align(g, guess)
    assert r0["stats"]["passes_timed"] == 0 and r0["stats"]["pass_ms_total"] == 0
    assert _same(r0, r)
    g.close()


def _poses(guess):
    g = np.asarray(guess, np.float64)
    out = []
    for dx in (0.0, 0.25, -0.5):
        p = g.copy()
        p[0, 3] += dx
        out.append(p)
    return np.stack(out)


@pytest.mark.parametrize("voxel", [False, True], ids=["exact", "voxelized"])
def test_zero_iterations_returns_the_guess(rig_guess, voxel):
    """setMaximumIterations(0) through align and through the batch: every lane is its guess cast through float, nothing is launched."""
    rig, guess = rig_guess
    g = _handle(rig, voxel=voxel)
    g.setMaximumIterations(0)
    r = _align(g, guess)
    assert np.array_equal(r["T"], np.asarray(guess, np.float32)) and r["it"] == 0 and not r["conv"]
    assert np.array_equal(r["H"], np.eye(6))
    s = r["stats"]
    assert s["passes"] == 0 and r["trace"].shape[0] == 0 and s["loop_ms"] == 0
    assert s["passes_timed"] == 0 and s["host_wait_spins"] == 0
    G = _poses(guess)
    T, conv, its, H = (g.alignBatchVoxel if voxel else g.alignBatch)(G)
    assert np.array_equal(T, G.astype(np.float32)) and not conv.any() and (its == 0).all()
    assert all(np.array_equal(H[i], np.eye(6)) for i in range(len(G)))
    assert all(g.lm_trace(lane=i).shape[0] == 0 for i in range(len(G)))
    s2 = g.stats()  # (the batch leaves the last align's statistics alone)
    assert s2["passes"] == 0 and s2["loop_ms"] == 0
    g.close()


def test_voxelized_align_leaves_the_exact_path_alone(rig_guess):
    """exact, voxelized, exact on one handle against exact, exact on another: the voxelized align reports staged_fraction 0 and touches
    neither the share of listed queries the next exact align decides its first pass by nor the launch order the handle carries."""
    rig, guess = rig_guess
    a, b = _handle(rig), _handle(rig)
    ra, rb = _align(a, guess), _align(b, guess)
    assert _same(ra, rb) and ra["stats"]["staged_fraction"] == rb["stats"]["staged_fraction"]
    a.setVoxelResolution(VOXEL_RES)
    rv = _align(a, guess)
    assert rv["stats"]["staged_fraction"] == 0 and rv["stats"]["passes"] > 0
    a.setVoxelResolution(0.0)
    for g in (a, b):  # the first pass alone: its staged_fraction is the alignment's
        g.setMaximumIterations(1)
    fa, fb = _align(a, guess), _align(b, guess)
    print(f"first-pass staged_fraction {fa['stats']['staged_fraction']!r} / {fb['stats']['staged_fraction']!r}; full {ra['stats']['staged_fraction']!r}")
    assert _same(fa, fb) and fa["stats"]["passes"] == fb["stats"]["passes"] and fa["stats"]["staged_fraction"] == fb["stats"]["staged_fraction"]
    for g in (a, b):
        g.setMaximumIterations(rig.max_iter)
    ga, gb = _align(a, guess), _align(b, guess)
    assert _same(ga, gb) and _same(ga, ra) and ga["stats"]["staged_fraction"] == gb["stats"]["staged_fraction"]
    a.close()
    b.close()
