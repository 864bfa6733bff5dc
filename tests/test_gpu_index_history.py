"""The index a long-lived handle really builds (-m gpu): grid rows and cells crowded past the search's 16-bit fields, index objects
recycled at the same address, and voxels taken from the auto-voxel memo.  The inputs are tests/_index_history_cases.py's;
tests/test_index_history_cases_cpu.py shows on the CPU that they do what is claimed here.

A. Crowded rows and cells.  ngicp_pass_group.inc packs, per listed region row, where the batch box's x-cells begin and end as two
   16-bit fields saturated at 0xffff (a start HINT of the row's walk, which covers the whole row either way), and clamps the start
   hint of a ring-1 unit to 22 bits; ngicp_pass_st.h keeps the first eight cell bounds of a row as unsigned short, saturated: a
   saturated lower bound is still a superset, a saturated upper bound is replaced by the row's end (`if (rbnd == 0xffff) rbnd = n`).
   crowded_cell has 70 000 target points in one cell, crowded_row 35 000 in each of five cells of one row.
   A batch lists its region's rows only when the rings that cover the gate number two or more (ngicp_align.h: stage_grow), so the
   packed fields are read in the runs without a gate; with the 1 m gate (one ring at these voxels) the ring-1 units and their hint
   serve every query.  Both are run, and stats()'s staged_fraction is asserted to say which happened.
B. Recycled index objects: with the process-wide pool drained, a release followed by a build hands the handle the same object
   (stats()'s device_allocs does not grow), whose buffers still hold the previous cloud's index.
C. The memo chain: a handle indexes a new cloud with the voxel of the last cloud of similar size; the occupancy check is deferred
   and corrects the memo for the next build only.  Results must stay exact (the oracle is the reference: under another voxel the
   summation order differs from a fresh handle's) while the voxel is wrong by a factor of more than 4 in either direction."""
import gc
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _index_history_cases as ic
from _pass_check import _configure, _crowded_rig, check_passes, handle_env
from test_gpu_batch import _assert_lanes_equal, _single
from test_gpu_queries import DBL_MAX, _check_fitness, _check_radius, _d2_rows, _nn_d2, _transformed
from test_gpu_search_matrix import _caps, _check_covariances, _check_knn, _queries
from test_gpu_variants import ROOT, SWITCHES, VARIANTS, WORKER

pytestmark = pytest.mark.gpu

GATES = {"gate1": 1.0, "nogate": None}
HANDLE_ENVS = {
    "default": {},
    "persist": {"NGICP_PERSIST": "1"},
    "head": {"NGICP_HEAD": "1"},
    "cell_boxes": {"NGICP_CELL_BOXES": "1"},
    "grow0": {"NGICP_STAGE_GROW": "0"},
    "grow2": {"NGICP_STAGE_GROW": "2"},
    "grow6": {"NGICP_STAGE_GROW": "6"},
}


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _iso(n):
    return np.repeat(ic.ISO_COV[None], n, 0)


def _d2_all(pts, q, chunk=50):
    """_d2_rows of every query, a few rows at a time (its temporaries are three times the result)."""
    pts = np.ascontiguousarray(pts[:, :3], np.float32)
    D = np.empty((len(q), len(pts)), np.float32)
    for s in range(0, len(q), chunk):
        D[s:s + chunk] = _d2_rows(pts, q[s:s + chunk])
    return D


def _pick_queries(pts, h, seed, n, n_far=None):
    """n of _queries' points: half of them cloud points under a pose, the rest snapped onto cell faces, and the far ones (all 42, or
    n_far of them spread over directions and distances)."""
    if len(pts) < 300:  # (_queries draws 300 distinct cloud points)
        far = pts.mean(0) + np.array([[1e3, 0, 0], [0, -1e3, 0], [7e2, 7e2, -7e2], [-1e4, 0, 0]])
        q = np.r_[pts + np.float32(0.01), pts, far][:n]
        assert len(q) == n
        return np.ascontiguousarray(q.astype(np.float32))
    q, n_near = _queries(pts, h, np.random.default_rng(seed))
    far = np.arange(n_near, len(q))
    if n_far is not None:
        far = far[np.linspace(0, len(far) - 1, n_far).astype(int)]
    n_moved = n // 2
    idx = np.r_[0:n_moved, 300:300 + (n - n_moved - len(far)), far]
    assert len(idx) == n
    return np.ascontiguousarray(q[idx])


# ================================================================== A. crowded rows and cells
@pytest.mark.parametrize("env", list(HANDLE_ENVS))
@pytest.mark.parametrize("gate", list(GATES))
@pytest.mark.parametrize("case", list(ic.CROWDED))
def test_crowded_every_pass(ng, oracle_mod, case, gate, env):
    """Every pass of an alignment against the oracle and a fresh handle, on the default route and under each per-handle switch.
    Without a gate the batches list their region's rows (staged_fraction > 0: the packed fields were read) unless NGICP_STAGE_GROW=0
    forbids it; with the 1 m gate one ring covers the gate and nothing is listed."""
    rig, guess = _crowded_rig(ng, oracle_mod, case, env=HANDLE_ENVS[env], gate=GATES[gate])
    out = rig.run(guess, f"{case} {gate} {env}", fresh=True)
    s = rig.g.stats()
    first = rig.first_align_stats(guess)["staged_fraction"]
    print(f"{case} {gate} {env}: grid {s['grid_dims']}, voxel {s['voxel_size']}, passes {len(out)}, staged fraction {first:.4f} (first alignment), {s['staged_fraction']:.4f} (last)")
    assert s["grid_dims"] == ic.CROWDED[case][1] and s["voxel_size"] == np.float32(ic.CROWDED[case][0])
    assert s["n_tgt"] == len(rig.tgt) > ic.FIELD_MAX and len(out) >= 2
    if gate == "nogate" and env != "grow0":
        assert first > 0.0
    else:
        assert first == 0.0 and s["staged_fraction"] == 0.0
    rig.g.close()


CROWDED_VARIANTS = ("staged-wps3", "staged-wps4", "queue-wps3", "fused-wps3")
CROWDED_BUDGET_S = 60  # per case and child: above the engine's own 30 s stall report
_stopped = []  # the child that died by a signal or timed out: nothing more is started after it


@pytest.mark.parametrize("name", CROWDED_VARIANTS)
def test_crowded_every_pass_under_process_variant(hip_lib, oracle_mod, name):
    """tests/_variant_worker.py on the two crowded cases (make_rig: no gate, so that the default pass kernel's derivatives list their
    rows and the staged route meets rows of up to five crowded cells), a child per variant, one at a time; as in
    test_gpu_variants.py a child that dies by a signal or runs out of time stops the rest."""
    if _stopped:
        pytest.skip(f"not started: the child of variant {_stopped[0]} ended abnormally")
    cases = list(ic.CROWDED)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(VARIANTS[name])
    timeout = CROWDED_BUDGET_S * len(cases)
    try:
        res = subprocess.run([sys.executable, WORKER, *cases], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _stopped.append(name)
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"{name}: no result after {timeout} s\n{out[-3000:]}")
    if res.returncode < 0:
        _stopped.append(name)
    assert res.returncode == 0, f"{name} ({VARIANTS[name]}): exit {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print(name, json.dumps(out["cases"]))
    assert out["variant"] == VARIANTS[name]
    assert sorted(out["cases"]) == sorted(cases) and all(c["passes"] >= 2 for c in out["cases"].values())


# a squared radius that returns more than 65 535 neighbours from the cloud's centre, and one that returns a handful
CROWDED_RADII = {"crowded_cell": (12.5, 0.1 ** 2), "crowded_row": (1.5 ** 2, 0.03 ** 2)}


@pytest.mark.parametrize("case", list(ic.CROWDED))
def test_crowded_queries(ng, oracle_mod, case):
    """k-NN on both slots, radius search with more than 65 535 results and with a handful, fitness with and without a range, against
    numpy brute force in the engine's association."""
    voxel, dims, guess = ic.CROWDED[case]
    src, tgt = ic.CROWDED_CLOUDS[case]()
    g = ng.NanoGICP()
    g.setTuning(voxel)
    g.setInputSource(src); g.setInputTarget(tgt)
    g.setMaximumIterations(1)
    g.align(np.asarray(guess, np.float32))
    s = g.stats()
    assert s["grid_dims"] == dims and s["voxel_size"] == np.float32(voxel)
    q = _pick_queries(tgt, s["voxel_size"], 11, 300)
    for which, pts in (("target", tgt), ("source", src)):
        D = _d2_all(pts, q)
        for k in (1, 20, 32):
            _check_knn(g, which, pts, q, D, k)
    big, small = CROWDED_RADII[case]
    centre = (tgt.min(0) + tgt.max(0)) / 2
    qc = np.ascontiguousarray(np.r_[centre[None], q[:3], q[-2:]].astype(np.float32))
    n_ref = (_d2_all(tgt, qc) < np.float32(big)).sum(1)
    print(f"{case}: neighbours inside the large radius {n_ref.tolist()}")
    assert n_ref.max() > ic.FIELD_MAX
    off, _, _ = _check_radius(g, "target", tgt, qc, big)
    assert np.array_equal(np.diff(off), n_ref)
    off, _, _ = _check_radius(g, "target", tgt, q, small)
    n = np.diff(off)
    print(f"{case}: neighbours inside the small radius: median {np.median(n[:258])}, largest {n.max()}")
    assert 1 <= np.median(n[:150]) <= 20
    _check_radius(g, "source", src, q, small)
    T = np.asarray(guess, np.float32)
    d2 = _nn_d2(tgt, _transformed(g, oracle_mod, src, T))
    for max_range in (DBL_MAX, 0.05 ** 2):
        _, n_in = _check_fitness(g, d2, max_range, T)
        assert n_in > 0
    g.close()


@pytest.mark.parametrize("gate", list(GATES))
@pytest.mark.parametrize("case", list(ic.CROWDED))
def test_crowded_batch_lanes_are_the_single_aligns(ng, oracle_mod, case, gate):
    rig, guess = _crowded_rig(ng, oracle_mod, case, gate=GATES[gate])
    from direct_lidar_odometry_amd import clouds
    G = np.stack([np.asarray(guess, np.float32), np.eye(4, dtype=np.float32),
                  (np.asarray(guess, np.float64) @ clouds.make_pose((0.03, 0.02, -0.02), (0.5, 0.5, -1.0))).astype(np.float32)])
    f = rig.handle()
    for e in (rig.g, f):
        e.setMaximumIterations(rig.max_iter)
    refs = _single(f, G)
    f.close()
    print(f"{case} {gate}: single aligns: iterations {[r[2] for r in refs]}")
    _assert_lanes_equal(rig.g, rig.g.alignBatch(G), refs, f"{case} {gate}")
    assert len(rig.tgt) > ic.FIELD_MAX and max(r[2] for r in refs) >= 2
    rig.g.close()


def test_crowded_covariances(ng, oracle_mod):
    """The covariance k-NN with the 70 000-point cube as the source in ONE cell (voxel 1000): every point's 20 neighbours by brute
    force over the whole cloud, 4.9e9 distance tests."""
    _, tgt = ic.crowded_cell()
    g = ng.NanoGICP()
    g.setTuning(1000.0)
    g.setCorrespondenceRandomness(20)
    g.setInputSource(tgt)
    t0 = time.time()
    g.calculateSourceCovariances()
    covs = g.getSourceCovariances()
    t1 = time.time()
    n_full = _check_covariances(oracle_mod, tgt, covs, 20)
    print(f"crowded covariances: GPU {1e3 * (t1 - t0):.1f} ms (k-NN, covariances, read-back; covariance_ms {g.stats()['covariance_ms']:.2f}), reference {time.time() - t1:.2f} s")
    assert n_full > 60_000
    g.close()


# ================================================================== B. recycled index objects
def _drain_pool(ng):
    """Eight small clouds kept alive on helper handles: whatever the process-wide pool held (at most 8 objects) is now in use, so the
    next object released is the next one acquired.  The caller closes the handles at the end of its test."""
    gc.collect()  # (handles nobody closed give their objects back now, not between a release and a build of the test)
    rng = np.random.default_rng(9)
    helpers = []
    for _ in range(8):
        e = ng.NanoGICP()
        e.setInputSource(np.ascontiguousarray(rng.uniform(-1, 1, (64, 3)).astype(np.float32)))
        helpers.append(e)
    return helpers


def _close(handles):
    for e in handles:
        e.close()


RECYCLE_SETTINGS = dict(setTransformationEpsilon=1e-6, setRotationEpsilon=1e-6)
RECYCLE_ITER = 6


def _recycle_handle(ng, src, tgt, voxel=ic.RECYCLE_VOXEL, env=None, gate=1.0):
    with handle_env(env):
        g = ng.NanoGICP()
    g.setTuning(voxel)
    _configure(g, 20, gate, RECYCLE_SETTINGS)
    g.setInputSource(src); g.setInputTarget(tgt)
    g.setSourceCovariances(_iso(len(src))); g.setTargetCovariances(_iso(len(tgt)))
    return g


def _oracle(orc, src, tgt, gate=1.0):
    o = orc.OracleGICP()
    o.setNumThreads(16)
    _configure(o, 20, gate, RECYCLE_SETTINGS)
    o.setInputSource(src); o.setInputTarget(tgt)
    o.setSourceCovariances(_iso(len(src))); o.setTargetCovariances(_iso(len(tgt)))
    return o


def _run(g, o, guess, label, src, tgt, fresh=None, max_iter=RECYCLE_ITER):
    return check_passes(g, o, guess, label, src, tgt, _iso(len(src)), _iso(len(tgt)), max_iter, fresh=fresh)


def test_same_address_other_cloud_same_size(ng, oracle_mod):
    """align S1 -> T, then S2 (S1 mirrored, rows reversed: same n, same grid) on the SAME index object: the launch order the handle
    keeps per (object address, group count) - ngicp::order_src / order_groups, read in do_align - still describes S1's batches.
    Whether the group count is the same is not observable from outside; with the same n and the same grid it very likely is (it
    follows from the number of query batches), and if it is not, the host clears the order and the test checks the plain path.
    Every pass of S2 must match the oracle and a handle that never saw S1, bit for bit; the same through alignBatch, whose own
    order cache (BatchWs::order_src) has the same key."""
    from _pass_check import SHAPE_GUESS
    s1, s2, tgt = ic.recycle_pair()
    guess = np.asarray(SHAPE_GUESS, np.float32)
    G = np.stack([guess, np.eye(4, dtype=np.float32), np.asarray(SHAPE_GUESS @ SHAPE_GUESS, np.float32)])
    helpers = _drain_pool(ng)
    g = _recycle_handle(ng, s1, tgt)
    g.setMaximumIterations(RECYCLE_ITER)
    g.align(guess)
    g.alignBatch(G)
    assert g.stats()["passes"] > 1
    g.clearSourceCovariances()  # (they hold the index object they are ordered by)
    allocs = g.stats()["device_allocs"]
    g.setInputSource(s2)
    assert g.stats()["device_allocs"] == allocs  # no buffer was allocated: the object S1 was indexed in has come back
    g.setSourceCovariances(_iso(len(s2)))
    fresh = lambda: _recycle_handle(ng, s2, tgt)  # noqa: E731
    out = _run(g, _oracle(oracle_mod, s2, tgt), guess, "S2 on S1's object", s2, tgt, fresh=fresh)
    assert len(out) >= 2
    f = fresh()
    f.setMaximumIterations(RECYCLE_ITER)
    refs = _single(f, G)
    f.close()
    g.setMaximumIterations(RECYCLE_ITER)
    _assert_lanes_equal(g, g.alignBatch(G), refs, "alignBatch after align on S1's object")
    g.close()
    # the batch's own cache alone: no single align in between (the handles closed above have filled the pool again)
    helpers += _drain_pool(ng)
    b = _recycle_handle(ng, s1, tgt)
    b.setMaximumIterations(RECYCLE_ITER)
    b.alignBatch(G)
    b.clearSourceCovariances()
    allocs = b.stats()["device_allocs"]
    b.setInputSource(s2)
    assert b.stats()["device_allocs"] == allocs
    b.setSourceCovariances(_iso(len(s2)))
    _assert_lanes_equal(b, b.alignBatch(G), refs, "alignBatch on S1's object")
    b.close()
    _close(helpers)


@pytest.mark.parametrize("big", list(ic.BIG_THEN_TINY))
def test_big_then_tiny_on_one_object(ng, oracle_mod, big):
    """A 40-point index and a one-cell index built in an object whose buffers still hold a 175 000-point row / a grid at make_grid's
    cap: k-NN, radius search and every pass of an alignment see only the new cloud."""
    voxel = ic.BIG_THEN_TINY[big]
    first = ic.crowded_row()[1] if big == "crowded_row" else ic.memo_clouds()["wide"]
    rng = np.random.default_rng(12)
    helpers = _drain_pool(ng)
    g = ng.NanoGICP()
    g.setTuning(voxel)
    _configure(g, 5, None, RECYCLE_SETTINGS)
    g.setInputTarget(first)
    src = np.ascontiguousarray(first[:200] + np.float32(0.001))
    g.setInputSource(src)
    g.setMaximumIterations(1)
    g.align()
    s = g.stats()
    print(f"{big}: voxel {s['voxel_size']}, grid {s['grid_dims']}")
    _caps(s)
    if big == "wide":
        assert s["voxel_size"] > np.float32(voxel) and np.prod(s["grid_dims"]) > ic.MAX_CELLS // 4  # grown by make_grid to fit its cap
    else:
        assert s["grid_dims"] == [5, 1, 1]
    g.clearTargetCovariances()
    g.setTuning(ic.TINY_VOXEL[big])
    for name, tgt in zip(("40 points", "one cell"), ic.tiny_clouds()):
        allocs = g.stats()["device_allocs"]
        g.setInputTarget(tgt)
        assert g.stats()["device_allocs"] == allocs  # the big index's object, none of its buffers too small
        q = np.ascontiguousarray(np.r_[tgt + np.float32(0.004), tgt[:5], first[:20], rng.uniform(-3, 3, (40, 3))].astype(np.float32))
        D = _d2_all(tgt, q)
        for k in sorted({1, min(20, len(tgt)), min(32, len(tgt))}):
            _check_knn(g, "target", tgt, q, D, k)
        ext = float(np.ptp(tgt, 0).max())
        for radius in ((0.3 * ext) ** 2, (2.0 * ext) ** 2):
            _check_radius(g, "target", tgt, q, radius)
        noise = 0.02 if len(tgt) == 40 else 0.0005
        src = np.ascontiguousarray((tgt + rng.normal(0, noise, tgt.shape)).astype(np.float32))
        g.setInputSource(src)
        g.setSourceCovariances(_iso(len(src))); g.setTargetCovariances(_iso(len(tgt)))
        o = oracle_mod.OracleGICP()
        o.setNumThreads(16)
        _configure(o, 5, None, RECYCLE_SETTINGS)
        o.setInputSource(src); o.setInputTarget(tgt)
        o.setSourceCovariances(_iso(len(src))); o.setTargetCovariances(_iso(len(tgt)))
        _run(g, o, ic.MEMO_GUESS, f"{name} after {big}", src, tgt, max_iter=3)
        s = g.stats()
        print(f"{name} after {big}: voxel {s['voxel_size']}, grid {s['grid_dims']}")
        assert s["n_tgt"] == len(tgt)
        if name == "one cell":
            assert s["grid_dims"] == [1, 1, 1]
        g.clearTargetCovariances()
    g.close()
    _close(helpers)


def test_object_passes_between_handles_with_and_without_cell_boxes(ng, oracle_mod):
    """An index object built by an NGICP_CELL_BOXES=1 handle (per-cell boxes beside the cell starts) is released and rebuilt by a
    handle without the switch, and the other way round: the pass of each reads the boxes only when its own build made them."""
    from _pass_check import SHAPE_GUESS
    s1, s2, tgt = ic.recycle_pair()
    guess = np.asarray(SHAPE_GUESS, np.float32)
    helpers = _drain_pool(ng)
    boxes = {"NGICP_CELL_BOXES": "1"}
    a = _recycle_handle(ng, s1, tgt, env=boxes)
    b = _recycle_handle(ng, s2, tgt)
    oa, ob = _oracle(oracle_mod, s1, tgt), _oracle(oracle_mod, s2, tgt)
    # (no fresh handles yet: closing one would put ITS objects into the pool, in front of the one this test hands over)
    _run(a, oa, guess, "cell boxes, own object", s1, tgt)
    _run(b, ob, guess, "no cell boxes, own object", s2, tgt)
    # a's target object goes to the pool; b releases its own behind it and takes a's (the pool hands out the oldest)
    a.clearTarget()
    b.clearTargetCovariances()
    allocs = b.stats()["device_allocs"]
    t2 = tgt.copy()
    b.setInputTarget(t2)
    assert b.stats()["device_allocs"] == allocs
    b.setTargetCovariances(_iso(len(tgt)))
    _run(b, ob, guess, "no cell boxes, on the object a box handle built", s2, tgt, fresh=lambda: _recycle_handle(ng, s2, tgt))
    # the pool now holds the object b built without boxes and those of the fresh handles above, built without boxes as well: a takes
    # one of them (its box table is allocated now, or grown)
    t3 = tgt.copy()
    a.setInputTarget(t3)
    a.setTargetCovariances(_iso(len(tgt)))
    _run(a, oa, guess, "cell boxes, on the object a plain handle built", s1, tgt, fresh=lambda: _recycle_handle(ng, s1, tgt, env=boxes))
    a.close(); b.close()
    _close(helpers)


# ================================================================== C. the memo chain
MEMO_SETTINGS = dict(setTransformationEpsilon=1e-6, setRotationEpsilon=1e-6)


class _Chain:
    """One handle taken through a chain of targets (a copy of the cloud per step: a new identity, so a new build).  step(i) brings the
    handle to target i - building the targets before it if no test has yet - and returns what stats() said after its first alignment."""

    def __init__(self, ng, chain):
        self.ng, self.chain, self.clouds = ng, chain, ic.memo_clouds()
        self.src = self.clouds["source"]
        self.g = None
        self.seen = []  # (name, voxel, grid) per step built
        self.tgt = None
        self.kept = []  # every copy stays alive: a cloud's identity is its address

    def step(self, i):
        if self.g is None:
            self.g = self.ng.NanoGICP()
            _configure(self.g, 20, 1.0, MEMO_SETTINGS)
            self.g.setInputSource(self.src)
            self.g.setSourceCovariances(_iso(len(self.src)))
        assert len(self.seen) <= i + 1, "the chain only moves forward"
        while len(self.seen) <= i:
            name = self.chain[len(self.seen)]
            self.tgt = self.clouds[name].copy()
            self.kept.append(self.tgt)
            self.g.setInputTarget(self.tgt)
            self.g.setTargetCovariances(_iso(len(self.tgt)))
            self.g.setMaximumIterations(1)
            self.g.align(np.asarray(ic.MEMO_GUESS, np.float32))
            s = self.g.stats()
            _caps(s)
            self.seen.append((name, s["voxel_size"], s["grid_dims"]))
            print(f"memo chain step {len(self.seen) - 1}: {name}: voxel {s['voxel_size']:.4f}, grid {s['grid_dims']}")
        return self.seen[i]


_chains = {}
_fresh = {}


def _chain(ng, which):
    if which not in _chains:
        _chains[which] = _Chain(ng, ic.MEMO_CHAIN if which == "chain" else ic.MEMO_REVERSE)
    return _chains[which]


def _fresh_voxel(ng, name):
    """(voxel, grid) of the cloud as the FIRST cloud a handle indexes."""
    if name not in _fresh:
        c = ic.memo_clouds()
        f = ng.NanoGICP()
        _configure(f, 20, 1.0, MEMO_SETTINGS)
        f.setInputTarget(c[name])
        f.setInputSource(c["source"])  # (3 000 points: not the size class of the 12 000 / 15 000 targets)
        f.setMaximumIterations(1)
        f.align(np.asarray(ic.MEMO_GUESS, np.float32))
        s = f.stats()
        _fresh[name] = (s["voxel_size"], s["grid_dims"])
        f.close()
    return _fresh[name]


MEMO_STEPS = [("chain", i) for i in range(len(ic.MEMO_CHAIN))] + [("reverse", i) for i in range(len(ic.MEMO_REVERSE))]


@pytest.mark.parametrize("which,i", MEMO_STEPS, ids=[f"{w}-{i}-{(ic.MEMO_CHAIN if w == 'chain' else ic.MEMO_REVERSE)[i]}" for w, i in MEMO_STEPS])
def test_memo_chain_stays_exact(ng, oracle_mod, which, i):
    """After every target of the chain: the grid respects make_grid's caps, k-NN and radius search on the target slot equal brute
    force, and every pass of a short alignment matches the oracle."""
    ch = _chain(ng, which)
    name, h, dims = ch.step(i)
    g, tgt, src = ch.g, ch.tgt, ch.src
    # Far queries: four, not _queries' 42, and none on the 20 M cells of the wide cloud under the dense cloud's voxel.  A query outside
    # the grid is exact there too, but one lane pair then visits every row of every ring, ring after ring: measured 4.3 s per call
    # however few such queries there are (tests/test_gpu_search_matrix.py covers far queries on grids at make_grid's cap).
    q = _pick_queries(tgt, h, 100 + i, 200, n_far=4 if np.prod(dims) <= 1 << 20 else 0)
    D = _d2_all(tgt, q)
    t0 = time.time()
    for k in (1, 20):
        _check_knn(g, "target", tgt, q, D, k)
    t1 = time.time()
    _check_radius(g, "target", tgt, q, float(min((2.5 * h) ** 2, 2.0 ** 2)))
    print(f"{which} step {i}: k-NN checks {t1 - t0:.2f} s, radius check {time.time() - t1:.2f} s")
    o = oracle_mod.OracleGICP()
    o.setNumThreads(16)
    _configure(o, 20, 1.0, MEMO_SETTINGS)
    o.setInputSource(src); o.setInputTarget(tgt)
    o.setSourceCovariances(_iso(len(src))); o.setTargetCovariances(_iso(len(tgt)))
    out = check_passes(g, o, ic.MEMO_GUESS, f"{which} step {i} ({name}, voxel {h:.4f}, grid {dims})", src, tgt, _iso(len(src)), _iso(len(tgt)), 3)
    assert len(out) >= 1 and g.stats()["voxel_size"] == h  # (the alignments built nothing anew)


def test_memo_hits_recovers_and_wraps(ng):
    """The first build of a size class on an aged handle takes the other cloud's voxel: off by more than a factor of 4 (the CPU
    restatement: x23 too small for the wide cloud, a single cell for the dense one).  Every further build of the class is strictly
    closer to a fresh handle's voxel: the deferred occupancy read-back (count_and_scan(.., occ_device_only)) corrects the memo for the
    next build, by at most a factor of 4.
    Four slots, first in first out: n90000 is the fifth class after the source's 3 000 (which n2000 joins), 12-15k, n500 and n40000;
    it takes the oldest slot, the source's.  The 12-15k class SURVIVES that, so the dense cloud after n90000 is still a memo hit,
    at the voxel the wide clouds left there (far too large).  n150 then evicts it, and the dense cloud after n150 is indexed exactly
    like the very first one."""
    ch, rv = _chain(ng, "chain"), _chain(ng, "reverse")
    ch.step(len(ic.MEMO_CHAIN) - 1)
    rv.step(len(ic.MEMO_REVERSE) - 1)
    fd, fw = _fresh_voxel(ng, "dense"), _fresh_voxel(ng, "wide")
    print("fresh handles: dense", fd, "wide", fw)
    print("chain:", ch.seen)
    print("reverse:", rv.seen)
    assert [s[0] for s in ch.seen] == list(ic.MEMO_CHAIN) and [s[0] for s in rv.seen] == list(ic.MEMO_REVERSE)
    assert ch.seen[0][1:] == fd and rv.seen[0][1:] == fw  # the first target of either handle is a first build
    # the first hit is real
    assert fw[0] / ch.seen[1][1] > 4 and np.prod(ch.seen[1][2]) > 1 << 24
    assert rv.seen[1][1] / fd[0] > 4 and rv.seen[1][2] == [1, 1, 1]
    # ... and every further build is strictly closer
    for seen, ref in ((ch.seen[1:4], fw[0]), (rv.seen[1:4], fd[0])):
        off = [abs(np.log(h / ref)) for _, h, _ in seen]
        assert off[0] > off[1] > off[2], off
    # the slots wrap
    assert ch.seen[8][0] == "dense" and ch.seen[8][1] / fd[0] > 4      # the class survived n90000: still the wide clouds' voxel
    assert ch.seen[10][0] == "dense" and ch.seen[10][1:] == ch.seen[0][1:] == fd  # evicted by n150: a first build again
