"""The rolling voxel map's record routes on the GPU (ngicp_voxel_rolling_set / _insert_voxels / _insert_map / _transform; k_rollrec_keys /
k_rollrec_lookup / k_roll_commit / k_rollrec_fill in csrc/ngicp_voxel_roll.h) against the numpy model of their definition
(tests/_vgicp_rollmap_model.py, which proves itself in test_vgicp_rollmap_model_cpu.py).

Everything is compared with np.array_equal: the library is built with -ffp-contract=off and the definition fixes the order of every
sum.  The only tolerances are those of tests/test_gpu_vgicp_rolling.py for what a pass computes (H, b, err within 1e-9)."""
import numpy as np
import pytest

import _vgicp_model as vm
import _vgicp_nbr_model as nm
import _vgicp_rollmap_fixtures as fx
import _vgicp_rollmap_model as rm
from _vgicp_rolling_model import Refused

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -2, -3
I4 = fx.I4
TILE = 4096  # kScanTile (csrc/ngicp_grid.h): elements per block of the exclusive scan


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _handle(ng, res=fx.RES, K=1):
    g = ng.NanoGICP()
    g.setVoxelResolution(res)
    g.setNeighborSearchMethod(K)
    g.setVoxelRolling(True)
    return g


def _state(g):
    """(ijk, S, C, count, stamp, inserts, n_vox): the snapshot of _get and _stats that no refused call may change.  (Capacity and table
    slots are compared where a test means them: they are allocation, not state - two handles may reach one state by different routes.)"""
    st = g.voxelRollingStats()
    return (*g.rollingVoxelMap(), st["inserts"], st["n_vox"])


def _stats(g):
    return {k: v for k, v in g.voxelRollingStats().items() if not k.endswith("_ms")}


def _same(a, b, label):
    assert len(a) == len(b), label
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{label}: item {k} differs"


def _check(g, m, label):
    """the engine's state and the records its passes read against the model, bit for bit"""
    ijk, s, c, cnt, st, inserts, n_vox = _state(g)
    assert n_vox == len(ijk) == len(m), f"{label}: {len(ijk)} voxels, the model has {len(m)}"
    _same((ijk, s, c, cnt, st, inserts), (m.ijk, m.sum, m.covsum, m.count, m.stamp, m.inserts), label)
    stats = g.voxelRollingStats()
    assert stats["table_slots"] >= 2 * n_vox and stats["capacity_vox"] >= n_vox, f"{label}: {stats}"
    if len(m):
        _same(g.voxelMap(), (m.ijk, m.mean, m.cov, m.count), label + " (map records)")
    print(f"{label}: {len(m)} voxels, largest count {m.count.max() if len(m) else 0}, capacity {stats['capacity_vox']}, {stats['table_slots']} slots")
    return stats


def _raises(ng, code, fn, *a):
    with pytest.raises(ng.NgicpError) as e:
        fn(*a)
    assert e.value.code == code, f"{e.value}"
    return str(e.value)


def _built_engine(ng, K=1):
    """the map of fx.built_model on a handle, by scan inserts from a producer and one eviction"""
    d = fx.drive()
    prod, g = ng.NanoGICP(), _handle(ng, fx.RES, K)
    for s, c, T in zip(d["scans"][:3], d["covs"], d["poses"]):
        prod.setInputSource(s); prod.setSourceCovariances(c)
        g.insertIntoVoxelMap(prod, T)
    assert g.evictVoxelMap(**fx.EVICT) > 0
    return prod, g


# ---- 1. round trip -----------------------------------------------------------------------------------------------------------------------
def test_round_trip_restores_the_map_the_table_and_the_numbering(ng):
    d = fx.drive()
    prod, a = _built_engine(ng)
    saved = _state(a)
    assert len(saved[0]) > 1024 and set(saved[4].tolist()) == {1, 2, 3} and saved[5] == 3
    b = _handle(ng)
    b.setRollingVoxelMap(*saved[:6])
    _same(_state(b), saved, "get - set - get")
    _same(b.voxelMap(), a.voxelMap(), "the records the passes read")
    assert [x.dtype for x in _state(b)[:5]] == [x.dtype for x in saved[:5]]
    # the model restored from the same bytes is the model of the engine from here on
    m = rm.RecordVoxelMap(fx.RES)
    m.set(*saved[:6])
    _check(b, m, "restored")
    src, cs = d["scans"][3], d["covs"][3]
    guess = (d["gts"][3] @ fx.clouds.make_pose((0.05, -0.03, 0.02), (0.2, -0.3, 0.5))).astype(np.float32)
    for e in (a, b):  # (the source is the first cloud either handle indexes: tests/test_gpu_vgicp_rolling.py)
        e.setInputSource(src); e.setSourceCovariances(cs)
    for K in (1, 7, 27):
        out = []
        for e in (a, b):
            e.setNeighborSearchMethod(K)
            e.align(guess)
            out.append((e.getFinalTransformation().copy(), e.lm_trace().copy(), e.getFinalHessian().copy(), np.array([e.nr_iterations_, int(e.converged_)]),
                        e.voxel_correspondences()))
        _same(out[0], out[1], f"DIRECT{K}: the alignment on the restored handle")
        assert (out[0][4] >= 0).any() and out[0][3][0] > 0, f"DIRECT{K}"
    # a further scan insert and an eviction: the table and the numbering carry on alike
    prod.setInputSource(d["scans"][4]); prod.setSourceCovariances(d["covs"][4])
    got = [e.insertIntoVoxelMap(prod, d["poses"][4]) for e in (a, b)]
    assert got[0] == got[1] and got[0][0] > 0
    assert a.evictVoxelMap((0.0, 0.0, 0.0), 0.0, 3) == b.evictVoxelMap((0.0, 0.0, 0.0), 0.0, 3) > 0
    _same(_state(a), _state(b), "after a further insert and eviction")
    _same(a.voxelMap(), b.voxelMap(), "after a further insert and eviction (map records)")
    e = a.linearize(guess.astype(np.float64)), b.linearize(guess.astype(np.float64))
    _same((*e[0], a.voxel_correspondences()), (*e[1], b.voxel_correspondences()), "lookups through the rebuilt tables")
    # an empty state
    b.setRollingVoxelMap(*[x[:0] for x in saved[:5]], 7)
    assert _stats(b)["n_vox"] == 0 and _stats(b)["inserts"] == 7 and len(b.rollingVoxelMap()[0]) == 0
    _raises(ng, ERR_STATE, b.align, I4)
    for x in (prod, a, b):
        x.close()


# ---- 2. insert of records against the model -----------------------------------------------------------------------------------------------
def _records(res, n=None):
    _, S, C, cnt, _, _ = fx.built_records(res)
    return (S, C, cnt) if n is None else (S[:n], C[:n], cnt[:n])


def _insert_both(g, m, recs, T, label):
    got = g.insertVoxelsIntoVoxelMap(*recs, T)
    want = m.insert_records(*recs, T)
    assert got == want, f"{label}: (created, destination voxels) the engine {got}, the model {want}"
    return got


@pytest.mark.parametrize("n", [1, 37, 257, 3000, TILE - 1, TILE + 1])
def test_record_inserts_of_every_size_class_match_the_model(ng, n):
    """n records of the 0.5 m map into an empty 1 m map at the merging pose (0.3 rad, 1.3 m), then the same records again at identity
    into the map that now has some of their voxels."""
    recs = _records(0.5, n)
    assert len(recs[0]) == n
    g, m = _handle(ng), rm.RecordVoxelMap(fx.RES)
    created, touched = _insert_both(g, m, recs, fx.T_MERGE, "into an empty map")
    assert created == touched and (n < 200 or touched < n)  # records merge
    _check(g, m, f"{n} records into an empty map")
    created, touched = _insert_both(g, m, recs, I4, "into a map that has some of the voxels")
    assert n < 200 or 0 < created < touched
    st = _check(g, m, f"{n} records into a map that has some of the voxels")
    assert st["inserts"] == 2
    g.close()


def test_a_map_inserted_at_identity_into_an_empty_map_is_the_map(ng):
    """... at the identity and at a pose whose float image is the identity: S, C and n of every voxel bit for bit (the numbering is the
    insert's: ascending key)."""
    ijk, S, C, cnt, st, ins = fx.built_records()
    for T in (I4, fx.T_NEARLY_I):
        g, m = _handle(ng), rm.RecordVoxelMap(fx.RES)
        assert _insert_both(g, m, (S, C, cnt), T, "identity") == (len(ijk), len(ijk))
        _check(g, m, "a map at identity")
        gi, gs, gc, gn, gst = g.rollingVoxelMap()
        at = {tuple(k): v for v, k in enumerate(gi.tolist())}
        to = np.array([at[tuple(k)] for k in ijk.tolist()])
        _same((gs[to], gc[to], gn[to]), (S, C, cnt), "the map itself")
        assert (gst == 1).all()
        g.close()


def test_all_records_into_one_voxel(ng):
    """3000 records with means within a centimetre: one destination voxel, one thread adds a segment of 3000 in input order."""
    recs = fx.one_voxel_records(3000)
    g, m = _handle(ng), rm.RecordVoxelMap(fx.RES)
    assert _insert_both(g, m, recs, fx.T_MERGE, "one voxel") == (1, 1)
    _check(g, m, "3000 records into one voxel")
    assert _insert_both(g, m, recs, fx.T_MERGE, "one voxel again") == (0, 1)
    _check(g, m, "and again into the voxel that is there")
    assert g.rollingVoxelMap()[3][0] == 2 * int(recs[2].sum())
    g.close()


def test_one_insert_grows_the_arrays_and_doubles_the_table_twice(ng):
    ijk, S, C, cnt, st, ins = fx.built_records()
    g, m = _handle(ng), rm.RecordVoxelMap(fx.RES)
    g.setRollingVoxelMap(ijk[:300], S[:300], C[:300], cnt[:300], st[:300], ins)
    m.set(ijk[:300], S[:300], C[:300], cnt[:300], st[:300], ins)
    before = _check(g, m, "300 voxels restored")
    assert before["capacity_vox"] == 1024 and before["table_slots"] == 1024
    created, touched = _insert_both(g, m, _records(0.5), I4, "the 0.5 m map")
    after = _check(g, m, "after the insert")
    assert created > 724 and after["n_vox"] > 1024 and after["capacity_vox"] == 2048 and after["table_slots"] == 4 * before["table_slots"], (before, after)
    src = fx.drive()["scans"][3]
    g.setInputSource(src); g.setSourceCovariances(fx.drive()["covs"][3])
    g.linearize(np.eye(4))
    corr, _ = g.correspondences()
    assert np.array_equal(corr, m.lookup(src)) and (corr >= 0).any() and (corr < 0).any()  # every key is found in the rebuilt table
    g.close()


# ---- 3. handle to handle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_res,rolling_on", [(1.0, True), (0.5, True), (0.5, False)], ids=["same-resolution", "0.5m-into-1m", "rolling-off"])
def test_insert_map_equals_insert_voxels_of_the_fetched_records(ng, from_res, rolling_on):
    ijk, S, C, cnt, st, ins = fx.built_records(from_res)
    src = _handle(ng, from_res)
    src.setRollingVoxelMap(ijk, S, C, cnt, st, ins)
    before = _state(src)
    if not rolling_on:
        src.setVoxelRolling(False)  # (the map stays; only its sums are read)
    half = fx.built_records(1.0)
    a, b, m = _handle(ng), _handle(ng), rm.RecordVoxelMap(fx.RES)
    for e in (a, b, m):
        (e.setRollingVoxelMap if e is not m else e.set)(*[x[::2] for x in half[:5]], half[5])
    for T in (fx.T_MERGE, I4):
        got = a.insertVoxelMapFrom(src, T)
        _, fs, fc, fn, _ = src.rollingVoxelMap()  # fetched through the host
        assert got == b.insertVoxelsIntoVoxelMap(fs, fc, fn, T) == m.insert_records(fs, fc, fn, T)
        _same(_state(a), _state(b), "insert_map against insert_voxels")
        _same(a.voxelMap(), b.voxelMap(), "insert_map against insert_voxels (map records)")
    _check(a, m, "insert_map")
    if not rolling_on:
        src.setVoxelRolling(True)
    _same(_state(src), before, "the map that was read")
    for x in (src, a, b):
        x.close()


# ---- 4. move in place ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 7])
def test_transform_matches_the_model_and_keeps_the_ages(ng, K):
    d = fx.drive()
    recs = fx.built_records()
    g, m = _handle(ng, fx.RES, K), rm.RecordVoxelMap(fx.RES)
    g.setRollingVoxelMap(*recs)
    m.set(*recs)
    left = g.transformVoxelMap(fx.T_MERGE)
    assert left == m.transform(fx.T_MERGE) < len(recs[0])  # records merged
    st = _check(g, m, "moved")
    assert st["inserts"] == recs[5] and set(m.stamp.tolist()) == {1, 2, 3}  # the counter stays, the ages survive
    # an alignment's passes against the moved map, the guess moved likewise: H, b, err within 1e-9, voxel numbers exact
    src, cs = d["scans"][3], d["covs"][3]
    g.setInputSource(src); g.setSourceCovariances(cs)
    model = nm.VoxelGICPNbrModel.__new__(nm.VoxelGICPNbrModel)
    vm.NumpyGICP.__init__(model, src, src[:1], cs, cs[:1])  # (no target: the map is the rolling one)
    model.vmap = m
    model.set_neighbors(K)
    T = (fx.T_MERGE.astype(np.float64) @ d["gts"][3]).astype(np.float32).astype(np.float64)
    H, b, err = g.linearize(T)
    Hm, bm, em = model.linearize(T)
    assert np.array_equal(g.voxel_correspondences(), model.corr_n) and (model.corr_n >= 0).any()
    for got, want, what in ((H, Hm, "H"), (b, bm, "b"), ([err], [em], "err")):
        dd = np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max()
        print(f"DIRECT{K} {what}: off by {dd:.2e} of the largest entry")
        assert dd <= 1e-9, what
    T2 = (fx.clouds.make_pose((0.01, -0.02, 0.005), (0.1, 0.05, -0.2)) @ T).astype(np.float32).astype(np.float64)
    e2, m2 = g.compute_error(T2), model.compute_error(T2)
    assert abs(e2 - m2) <= 1e-9 * abs(m2), "compute_error"
    # eviction by age afterwards, and a scan insert into the moved map
    assert g.evictVoxelMap((0.0, 0.0, 0.0), 0.0, 2) == m.evict((0.0, 0.0, 0.0), 0.0, 2) > 0
    _check(g, m, "moved, then evicted by stamp")
    prod = ng.NanoGICP()
    prod.setInputSource(d["scans"][4]); prod.setSourceCovariances(d["covs"][4])
    Tn = (fx.T_MERGE.astype(np.float64) @ d["gts"][4]).astype(np.float32)
    assert g.insertIntoVoxelMap(prod, Tn) == m.insert(d["scans"][4], d["covs"][4], Tn)
    ijk, s, c, cnt, stp = g.rollingVoxelMap()
    assert np.array_equal(ijk, m.ijk) and np.array_equal(cnt, m.count) and np.array_equal(stp, m.stamp) and stp.max() == recs[5] + 1
    assert (np.abs(s - m.sum) <= 1e-12 * np.abs(m.sum)).all()  # (a scan insert: tests/test_gpu_vgicp_rolling.py's tolerance)
    # an empty map: a no-op
    g.clearVoxelMap()
    assert g.transformVoxelMap(fx.T_MERGE) == 0 and _stats(g)["inserts"] == 0
    prod.close(); g.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(ng):
    """The snapshot of _get and _stats (capacity and table slots included) before and after every refused call; then a valid call."""
    recs = fx.built_records()
    ijk, S, C, cnt, st, ins = recs
    g, m, other = _handle(ng), rm.RecordVoxelMap(fx.RES), _handle(ng)
    g.setRollingVoxelMap(*recs)
    m.set(*recs)
    other.setRollingVoxelMap(*recs)
    few = (S[:10], C[:10], cnt[:10])
    far = I4.copy(); far[0, 3] = 2.0 ** 21
    nan = S[:10].copy(); nan[4, 1] = np.nan
    dup = [np.concatenate([x, x[5:6]]) for x in recs[:5]]
    refused = [
        ("a moved mean out of range", ERR_ARG, lambda: g.insertVoxelsIntoVoxelMap(*few, far), lambda: m.insert_records(*few, far)),
        ("a map moved out of range", ERR_ARG, lambda: g.insertVoxelMapFrom(other, far), lambda: m.insert_records(S, C, cnt, far)),
        ("a transform out of range", ERR_ARG, lambda: g.transformVoxelMap(far), lambda: m.transform(far)),
        ("a NaN sum", ERR_ARG, lambda: g.insertVoxelsIntoVoxelMap(nan, C[:10], cnt[:10], I4), lambda: m.insert_records(nan, C[:10], cnt[:10], I4)),
        ("count 0", ERR_ARG, lambda: g.insertVoxelsIntoVoxelMap(S[:10], C[:10], np.where(np.arange(10) == 3, 0, cnt[:10]), I4),
         lambda: m.insert_records(S[:10], C[:10], np.where(np.arange(10) == 3, 0, cnt[:10]), I4)),
        ("no records", ERR_ARG, lambda: g.insertVoxelsIntoVoxelMap(S[:0], C[:0], cnt[:0], I4), lambda: m.insert_records(S[:0], C[:0], cnt[:0], I4)),
        ("duplicate ijk in set", ERR_ARG, lambda: g.setRollingVoxelMap(*dup, ins), lambda: m.set(*dup, ins)),
        ("a stamp above inserts", ERR_ARG, lambda: g.setRollingVoxelMap(ijk, S, C, cnt, st, ins - 1), lambda: m.set(ijk, S, C, cnt, st, ins - 1)),
        ("a stamp of 0", ERR_ARG, lambda: g.setRollingVoxelMap(ijk, S, C, cnt, st * 0, ins), lambda: m.set(ijk, S, C, cnt, st * 0, ins)),
        ("an index of 2^20", ERR_ARG, lambda: g.setRollingVoxelMap(np.where(np.arange(len(ijk))[:, None] == 3, 2 ** 20, ijk), S, C, cnt, st, ins),
         lambda: m.set(np.where(np.arange(len(ijk))[:, None] == 3, 2 ** 20, ijk), S, C, cnt, st, ins)),
        ("a count of 0 in set", ERR_ARG, lambda: g.setRollingVoxelMap(ijk, S, C, cnt * 0, st, ins), lambda: m.set(ijk, S, C, cnt * 0, st, ins)),
        ("negative inserts", ERR_ARG, lambda: g.setRollingVoxelMap(ijk[:0], S[:0], C[:0], cnt[:0], st[:0], -1), lambda: m.set(ijk[:0], S[:0], C[:0], cnt[:0], st[:0], -1)),
        ("from == h", ERR_ARG, lambda: g.insertVoxelMapFrom(g, I4), None),
    ]
    for label, code, call, model_call in refused:
        before, stats = _state(g), _stats(g)
        msg = _raises(ng, code, call)
        if model_call is not None:
            with pytest.raises(Refused):
                model_call()
        _same(_state(g), before, label)
        assert _stats(g) == stats, label
        if label == "duplicate ijk in set":
            assert f"rows 5 and {len(ijk)}" in msg, msg
        assert _insert_both(g, m, few, I4, label)[1] > 0  # a valid call still works
        _check(g, m, f"after '{label}' and a valid insert")
    # an empty `from`
    empty = _handle(ng)
    before = _state(g)
    _raises(ng, ERR_ARG, g.insertVoxelMapFrom, empty, I4)
    _same(_state(g), before, "an empty from")
    # the rolling setting off: NGICP_ERR_STATE from all four, and the map is as it was when it is switched on again
    g.setVoxelRolling(False)
    for call in (lambda: g.insertVoxelsIntoVoxelMap(*few, I4), lambda: g.insertVoxelMapFrom(other, I4), lambda: g.transformVoxelMap(I4), lambda: g.setRollingVoxelMap(*recs)):
        _raises(ng, ERR_STATE, call)
    g.setVoxelRolling(True)
    _same(_state(g), before, "the rolling setting off")
    none = ng.NanoGICP()  # no resolution set
    none.setVoxelRolling(True)
    _raises(ng, ERR_STATE, none.setRollingVoxelMap, *recs)
    _insert_both(g, m, few, fx.T_MERGE, "at the end")
    _check(g, m, "at the end")
    for x in (g, other, empty, none):
        x.close()


def test_a_voxels_count_stops_at_the_int_range(ng):
    """The limit is 2^31 - 1 (ngicp_voxel_rolling_get's count is an int): 2^30 fits; a second 2^30 would make 2^31 and is refused;
    2^30 - 1 reaches the limit exactly; one more point is refused.  Two inserts of 2^30 cannot both be accepted under that limit."""
    C = fx.spd(1, 6)[:, :3, :3]
    rec = lambda n: (np.array([[0.5, 0.5, 0.5]]) * n, C * n, np.array([n]))
    g, m = _handle(ng), rm.RecordVoxelMap(fx.RES)
    assert _insert_both(g, m, rec(2 ** 30), I4, "2^30") == (1, 1)
    for n, ok in ((2 ** 30, False), (2 ** 30 - 1, True), (1, False)):
        before, stats = _state(g), _stats(g)
        if ok:
            assert _insert_both(g, m, rec(n), I4, str(n)) == (0, 1)
        else:
            _raises(ng, ERR_ARG, g.insertVoxelsIntoVoxelMap, *rec(n), I4)
            with pytest.raises(Refused):
                m.insert_records(*rec(n), I4)
            _same(_state(g), before, f"a refused count of {n}")
            assert _stats(g) == stats
        _check(g, m, f"after a count of {n}")
    assert g.rollingVoxelMap()[3][0] == 2 ** 31 - 1
    three = tuple(np.concatenate([a, a, a]) for a in rec(2 ** 30))  # together past the limit, in a voxel that is new
    fresh = _handle(ng)
    _raises(ng, ERR_ARG, fresh.insertVoxelsIntoVoxelMap, *three, I4)
    assert _stats(fresh) == dict(inserts=0, n_vox=0, capacity_vox=0, table_slots=0)
    h = _handle(ng)  # the same through a move: two voxels of 2^30 squeezed into one
    two = (np.array([[0, 0, 0], [1, 0, 0]], np.int32), np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]]) * 2 ** 30, np.concatenate([C, C]), np.array([2 ** 30] * 2), np.array([1, 1]), 1)
    h.setRollingVoxelMap(*two)
    squeeze = I4.copy(); squeeze[0, 0] = 0.0
    before = _state(h)
    _raises(ng, ERR_ARG, h.transformVoxelMap, squeeze)
    _same(_state(h), before, "a refused move")
    for x in (g, fresh, h):
        x.close()


# ---- 6. isolation --------------------------------------------------------------------------------------------------------------------------
def test_the_record_entries_touch_nothing_else(ng):
    """The target slot, the last alignment's getters and ngicp_voxelmap_builds are untouched by all four entries; the hooks return
    NGICP_ERR_STATE until the next linearisation."""
    d = fx.drive()
    recs = fx.built_records()
    g, other = _handle(ng), _handle(ng)
    other.setRollingVoxelMap(*recs)
    src, cs = d["scans"][3], d["covs"][3]
    g.setInputSource(src); g.setSourceCovariances(cs)
    g.setInputTarget(d["scans"][5]); g.setTargetCovariances(d["covs"][5])  # (not read while the rolling setting is on)
    g.setRollingVoxelMap(*recs)
    g.align(d["poses"][3])

    def outside():
        return (g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.lm_trace().copy(), np.array([g.nr_iterations_, int(g.converged_)]),
                g.getTargetCovariances(), g.getSourceCovariances(), np.array([g.voxelMapBuilds()]))

    def stale():
        _raises(ng, ERR_STATE, g.compute_error, np.eye(4))
        _raises(ng, ERR_STATE, g.correspondences)
        _raises(ng, ERR_STATE, g.voxel_correspondences)

    want = outside()
    g.linearize(np.eye(4)); g.compute_error(np.eye(4))
    few = (recs[1][:50], recs[2][:50], recs[3][:50])
    for label, call in (("insert_voxels", lambda: g.insertVoxelsIntoVoxelMap(*few, fx.T_MERGE)), ("insert_map", lambda: g.insertVoxelMapFrom(other, I4)),
                        ("transform", lambda: g.transformVoxelMap(fx.T_MERGE)), ("set", lambda: g.setRollingVoxelMap(*recs))):
        call()
        stale()
        _same(outside(), want, label)
        g.linearize(np.eye(4)); g.compute_error(np.eye(4)); g.correspondences()
    assert g.voxelMapBuilds() == 0
    # with the setting off the handle aligns against its target as a handle that never had a rolling map
    g.setVoxelRolling(False)
    fresh = ng.NanoGICP()
    fresh.setVoxelResolution(fx.RES)
    fresh.setInputSource(src); fresh.setSourceCovariances(cs)
    fresh.setInputTarget(d["scans"][5]); fresh.setTargetCovariances(d["covs"][5])
    out = []
    for e in (g, fresh):
        e.align(d["poses"][3])
        out.append((*e.voxelMap(), e.getFinalTransformation().copy(), e.lm_trace().copy(), e.getFinalHessian().copy()))
    _same(out[0], out[1], "the target-based map after the record entries")
    for x in (g, other, fresh):
        x.close()
