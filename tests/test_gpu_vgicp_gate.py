"""The gated insert of the rolling voxel map (include/ngicp.h "rolling voxel map: gated insert", csrc/ngicp_voxel_gate.h) against the numpy
model of that definition (tests/_vgicp_gate_model.py) and against the engine's own plain insert and voxel fitness: the classes, the counts,
every array of rollingVoxelMap() and the counters of voxelRollingStats(), np.array_equal throughout.  The fixtures, and the proof that no
term of theirs sits on a gate, are in tests/test_vgicp_gate_model_cpu.py."""
import copy

import numpy as np
import pytest

import _vgicp_gate_model as gm
import _vgicp_rolling_model as rm
import _voxel_fitness_model as fm

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -2, -3
I4 = np.eye(4, dtype=np.float32)
COUNTS = ("n_points", "n_class", "n_kept", "n_new", "n_touched")


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture(scope="module")
def fixture_map():
    """the model's fixture map; never changed (the tests work on copies)"""
    return gm.build_map()


def _raises(ng, code, fn, *a, **kw):
    with pytest.raises(ng.NgicpError) as e:
        fn(*a, **kw)
    assert e.value.code == code, f"{e.value}"


def _state(m):
    """the model's map as setRollingVoxelMap takes it"""
    return m.ijk.astype(np.int32), m.sum.copy(), m.covsum.copy(), m.count.astype(np.int32), m.stamp.copy(), m.inserts


def _counters(g):
    s = g.voxelRollingStats()
    return {k: s[k] for k in ("inserts", "n_vox")}


def _same_map(g, m, label):
    ijk, s, c, cnt, st = g.rollingVoxelMap()
    assert np.array_equal(ijk, m.ijk), f"{label}: ijk / numbering"
    assert np.array_equal(cnt, m.count) and np.array_equal(st, m.stamp), f"{label}: counts / stamps"
    assert np.array_equal(s, m.sum), f"{label}: S"
    assert np.array_equal(c, m.covsum), f"{label}: C"
    assert _counters(g) == dict(inserts=m.inserts, n_vox=len(m)), f"{label}: {_counters(g)}"


def _same_engine_maps(a, b, label):
    for i, (x, y) in enumerate(zip(a.rollingVoxelMap(), b.rollingVoxelMap())):
        assert x.dtype == y.dtype and np.array_equal(x, y), f"{label}: array {i} of rollingVoxelMap()"
    assert _counters(a) == _counters(b), label


class Gate:
    """A handle with the rolling setting on, a producer that feeds it, and the model fed the same numbers."""

    def __init__(self, ng, K=7, res=gm.RES):
        self.ng, self.K = ng, K
        self.prod, self.g = ng.NanoGICP(), ng.NanoGICP()
        self.g.setVoxelResolution(res)
        self.g.setNeighborSearchMethod(K)
        self.g.setVoxelRolling(True)
        self.m = rm.RollingVoxelMap(res)

    def restore(self, m):
        self.m = copy.deepcopy(m)
        self.g.setRollingVoxelMap(*_state(m))

    def source(self, pts, covs, on=None):
        on = on or self.prod
        on.setInputSource(np.ascontiguousarray(pts, np.float32), identity=0)  # (0: always uploaded, whatever the array's address)
        on.setSourceCovariances(covs)

    def gated(self, pts, covs, T, gate, label="", **opt):
        """the engine's call against the model's -> the engine's result"""
        want = gm.gated_insert(self.m, pts, covs, T, self.K, gate, **opt)
        self.source(pts, covs)
        got = self.g.insertIntoVoxelMapGated(self.prod, T, gate, **opt)
        cls = self.g.voxelMapInsertClasses()
        assert cls.dtype == np.uint8 and np.array_equal(cls, want["cls"]), f"{label}: {int((cls != want['cls']).sum())} classes differ"
        assert [got[k] for k in COUNTS] == [want[k] for k in COUNTS], f"{label}: the engine {got}, the model {[want[k] for k in COUNTS]}"
        assert got["kernel_ms"] >= 0.0
        _same_map(self.g, self.m, label)
        return got

    def close(self):
        self.prod.close(); self.g.close()


@pytest.fixture(scope="module", params=gm.NEIGHBORS, ids=lambda K: f"DIRECT{K}")
def gate(ng, request):
    r = Gate(ng, request.param)
    yield r
    r.close()


# ---- the engine against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gm.SIZES)
def test_engine_against_model(gate, fixture_map, n):
    src, cv = gm.source(n)
    seen = np.zeros(4, np.int64)
    for max_m in gm.GATES:
        for min_count in (1, gm.FIX_MIN_COUNT):
            for flags in (1, 0):
                gate.restore(fixture_map)
                got = gate.gated(src, cv, gm.SRC_POSE, max_m, f"n {n}, gate {max_m:g}, min count {min_count}, flags {flags}", min_voxel_count=min_count,
                                 insert_new=flags, insert_unjudged=flags)
                seen += got["n_class"]
                if got["n_kept"] == 0:
                    assert (got["n_new"], got["n_touched"]) == (0, 0) and gate.m.inserts == fixture_map.inserts
    print(f"DIRECT{gate.K}, n = {n}: over the 16 calls {seen.tolist()} points NEW / EXPLAINED / CONFLICT / UNJUDGED")
    if n >= 255:
        assert (seen > 0).all()


@pytest.mark.parametrize("K", gm.NEIGHBORS)
def test_gated_inserts_in_a_row(ng, K):
    """stamps, numbering and the table carry over from one gated insert to the next, from an empty map on"""
    r = Gate(ng, K)
    for i, (n, T, max_m, opt) in enumerate(gm.RUN):
        src, cv = gm.source(n, seed=900 + i)
        got = r.gated(src, cv, T, max_m, f"DIRECT{K}, call {i}", **opt)
        print(f"DIRECT{K}, call {i}: {got['n_class']} kept {got['n_kept']}, {got['n_new']} new of {got['n_touched']} voxels, {len(r.m)} in the map")
    assert r.m.inserts == len(gm.RUN) - 1 and len(set(r.m.stamp.tolist())) > 1  # (one call of the run keeps nothing)
    r.close()


# ---- the anchor: the engine against the engine's own fitness and plain insert ----------------------------------------------------------------
@pytest.mark.parametrize("K", gm.NEIGHBORS)
def test_gated_insert_is_fitness_points_a_host_mask_and_a_plain_insert(ng, fixture_map, K):
    src, cv = gm.source(700)
    a, b = Gate(ng, K), Gate(ng, K)
    a.restore(fixture_map); b.restore(fixture_map)
    a.source(src, cv)
    got = a.g.insertIntoVoxelMapGated(a.prod, gm.SRC_POSE, gm.FIX_GATE)
    cls = a.g.voxelMapInsertClasses()
    # today's route on the second handle: score, download, mask, upload the subset as a source of its own, insert
    b.source(src, cv, on=b.g)
    m, _, v = b.g.voxel_fitness_points(gm.SRC_POSE)
    want = gm.classes_from_point_values(m, v, gm.FIX_GATE)
    keep = gm.kept(want)
    b.source(src[keep], cv[keep])
    n_new, n_touched = b.g.insertIntoVoxelMap(b.prod, gm.SRC_POSE)
    assert np.array_equal(cls, want)
    assert (got["n_kept"], got["n_new"], got["n_touched"]) == (int(keep.sum()), n_new, n_touched) and 0 < got["n_kept"] < 700
    _same_engine_maps(a.g, b.g, f"DIRECT{K}")
    a.close(); b.close()


# ---- identity: no gate is the plain insert; the plain insert is what it was ------------------------------------------------------------------
@pytest.mark.parametrize("own", [True, False], ids=["the handle is its own producer", "another handle produces"])
@pytest.mark.parametrize("populated", [False, True], ids=["empty map", "populated map"])
def test_no_gate_is_the_plain_insert(ng, fixture_map, own, populated):
    src, cv = gm.source(700)
    a, b = Gate(ng, 7), Gate(ng, 7)
    for r in (a, b):
        if populated:
            r.restore(fixture_map)
        r.source(src, cv, on=r.g if own else r.prod)
    got = a.g.insertIntoVoxelMapGated(a.g if own else a.prod, gm.SRC_POSE, gm.DBL_MAX)
    n_new, n_touched = b.g.insertIntoVoxelMap(b.g if own else b.prod, gm.SRC_POSE)
    assert (got["n_kept"], got["n_new"], got["n_touched"]) == (700, n_new, n_touched) and got["n_class"][gm.CONFLICT] == 0
    if not populated:
        assert got["n_class"] == [700, 0, 0, 0] and (a.g.voxelMapInsertClasses() == gm.NEW).all()
    _same_engine_maps(a.g, b.g, "no gate")
    a.close(); b.close()


def test_plain_insert_is_unchanged_around_the_feature(ng, fixture_map):
    """workspace isolation: the same plain insert before and after gated calls of other sizes on the same handle"""
    r = Gate(ng, 7)
    src, cv = gm.source(257)
    big, cvb = gm.source(4097)

    def plain():
        r.restore(fixture_map)
        r.source(src, cv)
        out = r.g.insertIntoVoxelMap(r.prod, gm.SRC_POSE)
        return out, r.g.rollingVoxelMap(), _counters(r.g)

    first = plain()
    r.restore(fixture_map)
    r.gated(big, cvb, gm.SRC_POSE, gm.FIX_GATE, "a larger gated insert", min_voxel_count=gm.FIX_MIN_COUNT)
    r.gated(src, cv, gm.SRC_POSE, 0.0, "a dry run", dry_run=1)
    again = plain()
    assert first[0] == again[0] and first[2] == again[2]
    for x, y in zip(first[1], again[1]):
        assert np.array_equal(x, y)
    r.m.insert(src, cv, gm.SRC_POSE)
    _same_map(r.g, r.m, "the plain insert against the model")
    r.close()


# ---- dry run, nothing kept, refusals ---------------------------------------------------------------------------------------------------------
def test_a_dry_run_classifies_and_leaves_everything_alone(ng, fixture_map):
    r = Gate(ng, 7)
    r.restore(fixture_map)
    src, cv = gm.source(700)
    own, cvo = gm.source(255)
    g = r.g
    guess = fm.pose((0.02, -0.01, 0.0), (0.1, 0.0, 0.2))
    # stats() reports the process's device allocations: two dry runs first, which size the workspace and both class arrays, and the
    # producer keeps the cloud it has from here on (an upload allocates too)
    for _ in range(2):
        want = r.gated(src, cv, gm.SRC_POSE, gm.FIX_GATE, "a dry run that sizes the buffers", dry_run=1, min_voxel_count=gm.FIX_MIN_COUNT)
    r.source(own, cvo, on=g)
    g.alignBatchVoxel(np.stack([np.eye(4), guess.astype(np.float64)]))
    g.align(guess)
    T = np.eye(4)
    g.linearize(T)

    def everything():
        return (g.rollingVoxelMap() + g.voxelMap(), g.voxelRollingStats(), g.stats(), g.compute_error(T), g.voxel_correspondences(), g.lm_trace().copy(), g.lm_trace(lane=1).copy(),
                g.getFinalTransformation().copy())

    everything()  # (the read-backs size their own buffers once)
    before = everything()
    dry = g.insertIntoVoxelMapGated(r.prod, gm.SRC_POSE, gm.FIX_GATE, dry_run=1, min_voxel_count=gm.FIX_MIN_COUNT)
    after = everything()
    dry_cls = g.voxelMapInsertClasses()
    assert [dry[k] for k in COUNTS] == [want[k] for k in COUNTS]  # (what the model gave above)
    for x, y in zip(before[0], after[0]):
        assert np.array_equal(x, y)
    assert before[1] == after[1] and before[2] == after[2] and before[3] == after[3]
    for x, y in zip(before[4:], after[4:]):
        assert np.array_equal(x, y)
    assert (dry["n_new"], dry["n_touched"]) == (0, 0) and 0 < dry["n_kept"] < 700
    real = r.gated(src, cv, gm.SRC_POSE, gm.FIX_GATE, "the same for real", min_voxel_count=gm.FIX_MIN_COUNT)
    assert [real[k] for k in COUNTS[:3]] == [dry[k] for k in COUNTS[:3]] and np.array_equal(g.voxelMapInsertClasses(), dry_cls) and real["n_touched"] > 0
    _raises(ng, ERR_STATE, g.compute_error, T)  # ... and the hooks' state is dropped by the call that inserts
    r.close()


def test_all_points_conflict(ng, fixture_map):
    r = Gate(ng, 7)
    r.restore(fixture_map)
    src, cv = gm.source(700)
    dense = np.arange(700) % 8 < 3  # the points on the dense floor: every one is judged, and a gate of 0 explains none
    got = r.gated(src[dense], cv[dense], gm.SRC_POSE, 0.0, "all CONFLICT")
    n = int(dense.sum())
    assert got["n_class"] == [0, 0, n, 0] and (got["n_kept"], got["n_new"], got["n_touched"]) == (0, 0, 0)
    assert _counters(r.g) == dict(inserts=fixture_map.inserts, n_vox=len(fixture_map)) and (r.g.voxelMapInsertClasses() == gm.CONFLICT).all()
    r.close()


def test_refusals_change_nothing(ng, fixture_map):
    r = Gate(ng, 7)
    g = r.g
    _raises(ng, ERR_STATE, g.voxelMapInsertClasses)  # before any call
    r.restore(fixture_map)
    src, cv = gm.source(257)
    r.gated(src, cv, gm.SRC_POSE, gm.FIX_GATE, "the accepted call", dry_run=1)
    cls0 = g.voxelMapInsertClasses()

    def unchanged(label):
        _same_map(g, r.m, label)
        assert np.array_equal(g.voxelMapInsertClasses(), cls0), f"{label}: the classes of the last accepted call"

    far = src.copy()
    far[3] = (5.0e5, 1.0, -1.0)  # has a voxel where it is, none 3e4 m further out: (5e5 + 3e4) / 0.5 > 2^20
    T_far = I4.copy(); T_far[0, 3] = 3.0e4
    r.source(far, cv)
    with pytest.raises(rm.Refused):
        gm.gated_insert(r.m, far, cv, T_far, 7, gm.FIX_GATE, insert_new=0)
    # its gate point has no cell either, so it is NEW and insert_new = 0 would drop it: the call refuses all the same
    _raises(ng, ERR_ARG, g.insertIntoVoxelMapGated, r.prod, T_far, gm.FIX_GATE, insert_new=0)
    unchanged("a point 2^20 voxels out that the gate would have dropped")
    T_nan = gm.SRC_POSE.copy(); T_nan[1, 3] = np.nan  # (a cloud with a NaN coordinate is refused at upload: the pose makes the point NaN)
    r.source(src, cv)
    _raises(ng, ERR_ARG, g.insertIntoVoxelMapGated, r.prod, T_nan, gm.FIX_GATE)
    unchanged("a NaN point")
    r.source(src, cv)
    for bad in (float("nan"), -1.0, float("inf")):
        _raises(ng, ERR_ARG, g.insertIntoVoxelMapGated, r.prod, gm.SRC_POSE, bad)
        unchanged(f"max_mahalanobis {bad}")
    _raises(ng, ERR_ARG, g.insertIntoVoxelMapGated, r.prod, gm.SRC_POSE, gm.FIX_GATE, min_voxel_count=0)
    unchanged("min_voxel_count 0")
    with pytest.raises(TypeError):
        g.insertIntoVoxelMapGated(r.prod, gm.SRC_POSE, gm.FIX_GATE, min_count=2)
    empty = ng.NanoGICP()
    _raises(ng, ERR_ARG, g.insertIntoVoxelMapGated, empty, gm.SRC_POSE, gm.FIX_GATE)  # a producer without a source
    unchanged("an empty source")
    empty.close()
    g.setVoxelRolling(False)
    _raises(ng, ERR_STATE, g.insertIntoVoxelMapGated, r.prod, gm.SRC_POSE, gm.FIX_GATE)
    g.setVoxelRolling(True)
    unchanged("the rolling setting off")
    got = r.gated(src, cv, gm.SRC_POSE, gm.FIX_GATE, "the handle still works")
    assert got["n_kept"] > 0
    g.clearVoxelMap()
    _raises(ng, ERR_STATE, g.voxelMapInsertClasses)  # a clear ends the classes' life
    # no resolution: a handle that never had one (setting it to 0 on the handle above would itself empty the map)
    h = ng.NanoGICP()
    h.setVoxelRolling(True)
    _raises(ng, ERR_STATE, h.insertIntoVoxelMapGated, r.prod, gm.SRC_POSE, gm.FIX_GATE)
    assert _counters(h) == dict(inserts=0, n_vox=0)
    _raises(ng, ERR_STATE, h.voxelMapInsertClasses)
    h.close(); r.close()


# ---- what it is for ----------------------------------------------------------------------------------------------------------------------------
def test_the_gate_keeps_part_of_a_moving_box_out_of_the_map(ng):
    """tests/_vgicp_ray_drive.py's room with the moving box, inserted at the true pose, ungated on one handle and gated on another.  The
    parameters, the cap and the expected figures are the model's (tests/test_vgicp_gate_model_cpu.py pins them)."""
    plain, gated = Gate(ng, gm.DRIVE_K, gm.DRIVE_RES), Gate(ng, gm.DRIVE_K, gm.DRIVE_RES)
    for f, (pose, pts, cv) in enumerate(gm.drive_frames()):
        plain.source(pts, cv)
        assert plain.g.insertIntoVoxelMap(plain.prod, pose) == plain.m.insert(pts, cv, pose)
        if f < gm.DRIVE_WARMUP:
            gated.source(pts, cv)
            assert gated.g.insertIntoVoxelMap(gated.prod, pose) == gated.m.insert(pts, cv, pose)
        else:
            got = gated.gated(pts, cv, pose, gm.DRIVE_GATE, f"frame {f}", min_voxel_count=gm.DRIVE_MIN_COUNT)
            print(f"frame {f}: {got['n_class']} NEW / EXPLAINED / CONFLICT / UNJUDGED, {got['kernel_ms']:.3f} ms")
    _same_map(plain.g, plain.m, "the ungated map")
    _same_map(gated.g, gated.m, "the gated map")
    trail_plain, trail_gated, lost, static = gm.drive_figures(plain.m, gated.m)
    print(f"{trail_plain} trail voxels without the gate, {trail_gated} with it; {lost} of {static} static voxels lost")
    assert trail_gated < trail_plain and lost <= gm.DRIVE_LOST_CAP
    plain.close(); gated.close()


# ---- the hot path reads what the gated insert left -------------------------------------------------------------------------------------------
def test_align_after_a_gated_insert_is_align_on_the_restored_snapshot(ng, fixture_map):
    r = Gate(ng, 7)
    r.restore(fixture_map)
    big, cvb = gm.source(4097)
    got = r.gated(big, cvb, gm.SRC_POSE, gm.FIX_GATE, "the insert", min_voxel_count=gm.FIX_MIN_COUNT)
    assert got["n_new"] > 0  # (new voxels entered the table)
    fresh = ng.NanoGICP()
    fresh.setVoxelResolution(gm.RES); fresh.setNeighborSearchMethod(7); fresh.setVoxelRolling(True)
    fresh.setRollingVoxelMap(*r.g.rollingVoxelMap(), r.g.voxelRollingStats()["inserts"])
    src, cv = gm.source(700)
    guess = fm.pose((0.03, -0.02, 0.004), (0.1, -0.1, 0.4))
    out = []
    for e in (r.g, fresh):
        e.setInputSource(src, identity=0); e.setSourceCovariances(cv)
        e.align(guess)
        out.append((e.getFinalTransformation().copy(), e.getFinalHessian().copy(), e.lm_trace().copy(), e.voxel_correspondences(), np.array([e.nr_iterations_, int(e.converged_)])))
    for i, (x, y) in enumerate(zip(*out)):
        assert np.array_equal(x, y), f"item {i} on the handle of the gated insert differs from the restored one"
    assert (out[0][3] >= 0).any()
    fresh.close(); r.close()
