"""tests/_vgicp_rollmap_model.py (the numpy restatement of the rolling map's record routes) held to properties that do not depend on
the engine, on the fixtures test_gpu_vgicp_rollmap.py uses."""
import numpy as np
import pytest

import _vgicp_rollmap_fixtures as fx
import _vgicp_rollmap_model as rm
from _vgicp_model import voxel_of
from _vgicp_rolling_model import Refused, rotate_sym, transform_pcl_f32


def _same(a, b):
    return a.snapshot() == b.snapshot()


@pytest.mark.parametrize("res", [0.5, 1.0])
def test_identity_insert_of_a_map_into_an_empty_map_is_the_map(res):
    """... bit for bit: S, C, n, the numbering apart (the insert numbers in ascending key).  Asserts on the way that every record's float
    mean lies in the record's own voxel - the condition the header names."""
    ijk, S, C, cnt, st, ins = fx.built_records(res)
    p = (S / cnt[:, None].astype(np.float64)).astype(np.float32)
    assert np.array_equal(voxel_of(p, res), ijk), "a float mean left its voxel"
    m = rm.RecordVoxelMap(res)
    assert m.insert_records(S, C, cnt, fx.I4) == (len(ijk), len(ijk))
    at = {tuple(k): v for v, k in enumerate(m.ijk.tolist())}
    to = np.array([at[tuple(k)] for k in ijk.tolist()])
    assert sorted(to.tolist()) == list(range(len(ijk)))
    assert np.array_equal(m.sum[to], S) and np.array_equal(m.covsum[to], C) and np.array_equal(m.count[to], cnt)
    assert (m.stamp == 1).all() and m.inserts == 1
    key = m.ijk[:, 2] * 2 ** 42 + m.ijk[:, 1] * 2 ** 21 + m.ijk[:, 0]
    assert (np.diff(key) > 0).all()  # new voxels in ascending (iz, iy, ix)
    # the same through a pose whose float image is the identity
    m2 = rm.RecordVoxelMap(res)
    m2.insert_records(S, C, cnt, fx.T_NEARLY_I)
    assert _same(m, m2)


def test_set_round_trip_and_refusals():
    ijk, S, C, cnt, st, ins = fx.built_records()
    built = fx.built_model()
    m = rm.RecordVoxelMap(fx.RES)
    m.set(ijk, S, C, cnt, st, ins)
    assert _same(m, built) and set(st.tolist()) == {1, 2, 3}
    d = fx.drive()
    for x in (m, built):  # the numbering and the counter carry on alike
        x.insert(d["scans"][4], d["covs"][4], d["poses"][4])
        x.evict((0.0, 0.0, 0.0), 0.0, 3)
    assert _same(m, built)
    before = m.snapshot()
    two = np.concatenate([ijk, ijk[5:6]])
    bad = [
        (two, *[np.concatenate([a, a[5:6]]) for a in (S, C, cnt, st)], ins),
        (np.where(np.arange(len(ijk))[:, None] == 3, 2 ** 20, ijk), S, C, cnt, st, ins),
        (ijk, S, C, np.where(np.arange(len(cnt)) == 7, 0, cnt), st, ins),
        (ijk, S, C, cnt, st, ins - 1),  # a stamp above the counter
        (ijk, S, C, cnt, np.where(np.arange(len(st)) == 2, 0, st), ins),
        (ijk, S, C, cnt, st, -1),
    ]
    for args in bad:
        with pytest.raises(Refused):
            m.set(*args)
        assert m.snapshot() == before
    with pytest.raises(Refused, match=f"rows 5 and {len(ijk)}"):
        m.set(*bad[0])
    m.set(ijk[:0], S[:0], C[:0], cnt[:0], st[:0], 9)
    assert len(m) == 0 and m.inserts == 9


def test_records_inserted_one_call_at_a_time_give_the_definitions_sums():
    """Each record into its own empty model: (s, c, N) spelled out here once more, from the header's text."""
    _, S, C, cnt, _, _ = fx.built_records()
    T = fx.T_MERGE
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    for r in range(0, len(S), 97):
        m = rm.RecordVoxelMap(fx.RES)
        assert m.insert_records(S[r:r + 1], C[r:r + 1], cnt[r:r + 1], T) == (1, 1)
        n = float(cnt[r])
        p = np.array([S[r, 0] / n, S[r, 1] / n, S[r, 2] / n]).astype(np.float32)
        q = transform_pcl_f32(T, p[None])
        assert np.array_equal(m.ijk, voxel_of(q, fx.RES))
        A, Cc = np.zeros(3) + S[r], np.zeros((3, 3)) + C[r]
        s = np.array([((R[k, 0] * A[0] + R[k, 1] * A[1]) + R[k, 2] * A[2]) + n * t[k] for k in range(3)])
        assert np.array_equal(m.sum[0], s) and np.array_equal(m.covsum[0], rotate_sym(R, Cc)) and m.count[0] == cnt[r] and m.stamp[0] == 1


def test_two_records_forced_into_one_voxel_add_in_input_order():
    """Three records with sums chosen so that the order of the additions shows: (a + b) + c differs from a + (b + c)."""
    res = 16.0  # (the heavy record's mean lies 2^23 m out: within 2^20 voxels of 16 m)
    S = np.array([[2.0 ** 53, 0.5, 0.5], [1.0, 0.5, 0.5], [1.0, 0.5, 0.5]])
    cnt = np.array([2 ** 30, 1, 1])  # means 2^23 / 1 / 1 on x: forced together by a pose that squeezes x
    T = np.eye(4, dtype=np.float32)
    T[0, 0] = 0.0
    C = fx.spd(3, 5)[:, :3, :3]
    m = rm.RecordVoxelMap(res)
    assert m.insert_records(S, C, cnt, T) == (1, 1)
    A = ((np.zeros(3) + S[0]) + S[1]) + S[2]
    assert A[0] == 2.0 ** 53 and (S[1, 0] + S[2, 0]) + S[0, 0] == 2.0 ** 53 + 2  # the order matters for these numbers
    R = T[:3, :3].astype(np.float64)
    assert np.array_equal(m.sum[0], [((R[k, 0] * A[0] + R[k, 1] * A[1]) + R[k, 2] * A[2]) + float(2 ** 30 + 2) * 0.0 for k in range(3)])
    assert np.array_equal(m.covsum[0], rotate_sym(R, ((np.zeros((3, 3)) + C[0]) + C[1]) + C[2])) and m.count[0] == 2 ** 30 + 2
    rev = rm.RecordVoxelMap(res)
    assert rev.insert_records(S[::-1], C[::-1], cnt[::-1], T) == (1, 1) and rev.sum[0, 1] == m.sum[0, 1]
    apart = rm.RecordVoxelMap(res)
    assert apart.insert_records(S, C, cnt, np.eye(4)) == (2, 2)  # (at identity the heavy record has a voxel of its own)
    assert np.array_equal(apart.sum[0], (np.zeros(3) + S[1]) + S[2]) and np.array_equal(apart.sum[1], S[0])


def test_a_voxels_count_stops_at_the_int_range():
    """The limit is 2^31 - 1 (the count of ngicp_voxel_rolling_get is an int).  2^30 fits; a second 2^30 would make 2^31 and is refused;
    2^30 - 1 reaches the limit exactly; after that one more point is refused.  A refusal writes nothing."""
    C = fx.spd(1, 6)[:, :3, :3]
    big = rm.RecordVoxelMap(1.0)
    rec = lambda n: (np.array([[0.5, 0.5, 0.5]]) * n, C * n, np.array([n]))
    assert big.insert_records(*rec(2 ** 30), np.eye(4)) == (1, 1)
    before = big.snapshot()
    with pytest.raises(Refused):
        big.insert_records(*rec(2 ** 30), np.eye(4))
    assert big.snapshot() == before
    assert big.insert_records(*rec(2 ** 30 - 1), np.eye(4)) == (0, 1) and big.count[0] == 2 ** 31 - 1 and big.inserts == 2
    before = big.snapshot()
    with pytest.raises(Refused):
        big.insert_records(*rec(1), np.eye(4))
    assert big.snapshot() == before
    # several records of one insert that pass the limit together, in a new voxel
    three = tuple(np.concatenate([a, a, a]) for a in rec(2 ** 30))
    fresh = rm.RecordVoxelMap(1.0)
    with pytest.raises(Refused):
        fresh.insert_records(*three, np.eye(4))
    assert len(fresh) == 0 and fresh.inserts == 0


def test_insert_refusals_write_nothing():
    m = fx.built_model()
    _, S, C, cnt, _, _ = fx.built_records()
    before = m.snapshot()
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 2.0 ** 21
    nan = S[:10].copy()
    nan[4, 1] = np.nan
    for args in ((S[:10], C[:10], cnt[:10], far), (nan, C[:10], cnt[:10], fx.I4), (S[:10], C[:10], np.where(np.arange(10) == 3, 0, cnt[:10]), fx.I4),
                 (S[:0], C[:0], cnt[:0], fx.I4)):
        with pytest.raises(Refused):
            m.insert_records(*args)
        assert m.snapshot() == before
    assert m.insert_records(S[:10], C[:10], cnt[:10], fx.I4) == (0, 10) and m.inserts == 4


def test_transform_then_evict_by_stamp_keeps_what_the_stamp_rule_says():
    m = fx.built_model()
    ijk, S, C, cnt, st, ins = fx.built_records()
    # what the rule says, from the records: a destination voxel's stamp is the largest stamp among the records whose moved mean it holds
    q = transform_pcl_f32(fx.T_MERGE, (S / cnt[:, None].astype(np.float64)).astype(np.float32))
    newest, total = {}, {}
    for k, s, n in zip(map(tuple, voxel_of(q, fx.RES).tolist()), st.tolist(), cnt.tolist()):
        newest[k] = max(newest.get(k, 0), s)
        total[k] = total.get(k, 0) + n
    left = m.transform(fx.T_MERGE)
    assert left == len(newest) < len(ijk), "the pose is meant to merge records"
    assert m.inserts == ins and {tuple(k): s for k, s in zip(m.ijk.tolist(), m.stamp.tolist())} == newest
    assert {tuple(k): n for k, n in zip(m.ijk.tolist(), m.count.tolist())} == total and m.count.sum() == cnt.sum()
    key = m.ijk[:, 2] * 2 ** 42 + m.ijk[:, 1] * 2 ** 21 + m.ijk[:, 0]
    assert (np.diff(key) > 0).all()
    gone = m.evict((0.0, 0.0, 0.0), 0.0, 3)
    assert gone == sum(1 for s in newest.values() if s < 3) > 0 and (m.stamp == 3).all() and len(m) == sum(1 for s in newest.values() if s == 3) > 0
    # moved there and back: not the original in general, and the header says so
    back = fx.built_model()
    back.transform(fx.T_MERGE)
    back.transform(np.linalg.inv(fx.T_MERGE.astype(np.float64)))
    assert back.count.sum() == cnt.sum() and len(back) < len(ijk)
    empty = rm.RecordVoxelMap(1.0)
    assert empty.transform(fx.T_MERGE) == 0 and empty.inserts == 0
