"""The listed-row ("far") units of the pass kernel (-m gpu): rows beyond ring 1 queued by ballot in the ring-1 unit format and drained by
the ring-1 drain (ngicp_pass_group.inc).  The inputs are tests/_far_units_cases.py's; tests/test_far_units_cases_cpu.py shows on the
CPU that they do what is claimed here: every query of the sandwich is 2.7 - 3.3 voxels from its neighbour, and its cold pass queues more
than kUnitCap units in some batch (more than one round).

Every pass of a short alignment (at most six) is compared with the oracle by tests/_pass_check.py (index up to exact ties, d2 bit for
bit, H and the errors), on the default route, under every per-handle switch and process-wide variant whose kernel holds the far section,
through alignBatch (k_gicp_pass_batch) and with a robust kernel (the ROBUST instantiation: against brute force, the oracle has none)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _far_units_cases as fc
from _pass_check import Rig, handle_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_far_units_worker.py")
HANDLE_ENVS = {"default": {}, "persist": {"NGICP_PERSIST": "1"}, "head": {"NGICP_HEAD": "1"}, "cell_boxes": {"NGICP_CELL_BOXES": "1"}}
# the process-wide variants whose pass kernel includes ngicp_pass_group.inc (tests/test_gpu_variants.py's switches)
VARIANTS = {
    "wps3": {"NGICP_PASS_WPS": "3"}, "wps4": {"NGICP_PASS_WPS": "4"},
    "fused-wps3": {"NGICP_FUSED": "1", "NGICP_PASS_WPS": "3"}, "fused-wps4": {"NGICP_FUSED": "1", "NGICP_PASS_WPS": "4"},
    "queue-wps3": {"NGICP_QUEUE": "1", "NGICP_PASS_WPS": "3"}, "queue-wps4": {"NGICP_QUEUE": "1", "NGICP_PASS_WPS": "4"},
}
SWITCHES = ("NGICP_PASS_IMPL", "NGICP_FUSED", "NGICP_QUEUE", "NGICP_ORDER", "NGICP_PASS_WPS")
CHILD_BUDGET_S = 90


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _iso(n):
    return np.repeat(fc.ISO_COV[None], n, 0)


def sandwich_rig(ng, orc, env=None, gate=fc.GATE, voxel=fc.VOXEL, src=None):
    s, tgt = fc.sandwich()
    src = s if src is None else src
    return Rig(ng, orc, src, tgt, 20, gate, fc.SETTINGS, covs=(_iso(len(src)), _iso(len(tgt))), tuning=voxel, env=env)


def brute_force(P, src, tgt):
    """Per source point under the float pose P: the smallest float32 squared distance to a target point, in the kernels' arithmetic
    (_pass_check.f32_sqd's), and the lowest target index that has it."""
    Tf = np.asarray(P, np.float32)
    p = src.astype(np.float32)
    q = [((Tf[r, 0] * p[:, 0] + Tf[r, 1] * p[:, 1]) + Tf[r, 2] * p[:, 2]) + Tf[r, 3] for r in range(3)]
    d = [q[r][:, None] - tgt[None, :, r].astype(np.float32) for r in range(3)]
    D = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return D.min(1), D.argmin(1)


def check_against_brute_force(where, P, cg, sg, src, tgt, gate):
    dmin, _ = brute_force(P, src, tgt)
    inside = dmin.astype(np.float64) < float(gate) ** 2 if gate is not None else np.ones(len(src), bool)
    assert np.array_equal(cg >= 0, inside), f"{where}: gate decisions differ"
    assert np.array_equal(sg[inside], dmin[inside]), f"{where}: squared distances differ from brute force"
    rows = np.flatnonzero(inside)  # (and the neighbour the GPU names really is at that distance)
    Tf = np.asarray(P, np.float32)
    p, t = src[rows].astype(np.float32), tgt[cg[rows]].astype(np.float32)
    d = [(((Tf[r, 0] * p[:, 0] + Tf[r, 1] * p[:, 1]) + Tf[r, 2] * p[:, 2]) + Tf[r, 3]) - t[:, r] for r in range(3)]
    assert np.array_equal((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], sg[rows]), f"{where}: a distance is not that of the neighbour named"


# ================================================================== every query far, more than one round
@pytest.mark.parametrize("env", list(HANDLE_ENVS))
def test_sandwich_every_pass(ng, oracle_mod, env):
    """Cold and warm passes with every query beyond ring 1, the cold one in more than one round; a fresh handle agrees on the default route."""
    rig = sandwich_rig(ng, oracle_mod, env=HANDLE_ENVS[env])
    out = rig.run(fc.GUESS, f"sandwich {env}", fresh=env == "default")
    last = rig.g.stats()
    first = rig.first_align_stats(fc.GUESS)
    print(f"sandwich {env}: grid {last['grid_dims']}, passes {len(out)}, staged fraction {first['staged_fraction']:.3f} (first alignment), {last['staged_fraction']:.3f} (last)")
    assert last["voxel_size"] == np.float32(fc.VOXEL) and 2 <= len(out) <= 6
    assert first["staged_fraction"] > 0.0 and last["staged_fraction"] > 0.0
    assert all(frac == 1.0 for _, frac, _, _ in out)  # (every query found its neighbour inside the gate: on a slab's face)
    rig.g.close()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_sandwich_and_ties_under_process_variant(hip_lib, oracle_mod, name):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(VARIANTS[name])
    res = subprocess.run([sys.executable, WORKER], capture_output=True, text=True, timeout=CHILD_BUDGET_S, env=env, cwd=ROOT)
    assert res.returncode == 0, f"{name} ({VARIANTS[name]}): exit {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print(name, json.dumps(out))
    assert out["variant"] == VARIANTS[name]


# ================================================================== no gate, a gate of one ring
def test_no_gate_lists_rows(ng, oracle_mod):
    rig = sandwich_rig(ng, oracle_mod, gate=None)
    out = rig.run(fc.GUESS, "sandwich, no gate", fresh=False)
    assert 2 <= len(out) <= 6 and rig.g.stats()["staged_fraction"] > 0.0 and rig.first_align_stats(fc.GUESS)["staged_fraction"] > 0.0
    rig.g.close()


def test_gate_of_one_ring_lists_nothing(ng, oracle_mod):
    """A 0.5 m voxel under the 0.5 m gate: one ring covers the gate, no batch lists rows, the far section does not run."""
    rig = sandwich_rig(ng, oracle_mod, voxel=0.5)
    out = rig.run(fc.GUESS, "sandwich, one ring", fresh=False)
    assert 2 <= len(out) <= 6 and rig.g.stats()["staged_fraction"] == 0.0 and rig.first_align_stats(fc.GUESS)["staged_fraction"] == 0.0
    assert rig.g.stats()["voxel_size"] == np.float32(0.5)
    rig.g.close()


# ================================================================== ties across rows
def check_ties(ng, env):
    src, tgt, winners = fc.ties()
    with handle_env(env):
        g = ng.NanoGICP()
    g.setTuning(fc.VOXEL)
    g.setMaxCorrespondenceDistance(fc.GATE)
    g.setInputSource(src); g.setInputTarget(tgt)
    g.setSourceCovariances(_iso(len(src))); g.setTargetCovariances(_iso(len(tgt)))
    g.setMaximumIterations(1)
    g.align(np.eye(4, dtype=np.float32))
    cg, sg = g.correspondences()
    s = g.stats()
    g.close()
    assert s["staged_fraction"] > 0.0 and s["voxel_size"] == np.float32(fc.VOXEL)
    assert np.array_equal(sg, np.full(len(src), 0.0625, np.float32))
    assert np.array_equal(cg, winners), f"the lower sorted position must win a tie: {np.flatnonzero(cg != winners).tolist()}"


@pytest.mark.parametrize("env", list(HANDLE_ENVS))
def test_tie_across_rows_goes_to_the_lower_position(ng, env):
    check_ties(ng, HANDLE_ENVS[env])


# ================================================================== short batches
@pytest.mark.parametrize("n", [1, 33, 45])
def test_short_batches(ng, n):
    """A single-query source, and sources whose last batch is short: the cold pass (every query far) against brute force."""
    full, tgt = fc.sandwich()
    src = np.ascontiguousarray(full[np.argsort(np.abs(full[:, :2] - full[0, :2]).max(1))[:n]])  # the n points nearest the first in (x, y)
    g = ng.NanoGICP()
    g.setTuning(fc.VOXEL)
    g.setMaxCorrespondenceDistance(fc.GATE)
    g.setInputSource(src); g.setInputTarget(tgt)
    g.setSourceCovariances(_iso(n)); g.setTargetCovariances(_iso(len(tgt)))
    g.setMaximumIterations(1)
    guess = np.asarray(fc.GUESS, np.float32)
    g.align(guess)
    cg, sg = g.correspondences()
    assert g.stats()["staged_fraction"] > 0.0
    g.close()
    check_against_brute_force(f"{n} queries", guess, cg, sg, src, tgt, fc.GATE)


# ================================================================== alignBatch, robust kernel
def test_batch_lanes_are_the_single_aligns(ng, oracle_mod):
    from direct_lidar_odometry_amd import clouds
    from test_gpu_batch import _assert_lanes_equal, _single
    rig = sandwich_rig(ng, oracle_mod)
    G = np.stack([np.asarray(fc.GUESS, np.float32), np.eye(4, dtype=np.float32),
                  (np.asarray(fc.GUESS, np.float64) @ clouds.make_pose((0.03, 0.02, -0.02), (0.5, 0.5, -1.0))).astype(np.float32)])
    f = rig.handle()
    for e in (rig.g, f):
        e.setMaximumIterations(rig.max_iter)
    refs = _single(f, G)
    f.close()
    _assert_lanes_equal(rig.g, rig.g.alignBatch(G), refs, "sandwich")
    assert max(r[2] for r in refs) >= 2
    rig.g.close()


def test_robust_instantiation_against_brute_force(ng, oracle_mod):
    """k_gicp_pass's ROBUST build: the pass a handle with a Huber kernel searched last, cold (m = 1) and warm (m = 2, 3), against brute force
    at the pose it searched at (the result of the alignment one iteration shorter)."""
    rig = sandwich_rig(ng, oracle_mod)
    g = rig.g
    g.setRobustKernel(ng.RobustKernel.HUBER, 0.5)
    P = np.asarray(fc.GUESS, np.float32)
    for m in (1, 2, 3):
        g.setMaximumIterations(m)
        g.align(np.asarray(fc.GUESS, np.float32))
        if g.nr_iterations_ + 1 < m:
            break  # (converged earlier: nothing new was searched)
        cg, sg = g.correspondences()
        check_against_brute_force(f"robust, pass {m}", P, cg, sg, rig.src, rig.tgt, fc.GATE)
        assert g.stats()["staged_fraction"] > 0.0
        P = g.getFinalTransformation().copy()
    g.close()
