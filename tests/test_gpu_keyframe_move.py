"""Moving keyframes on the GPU (ngicp_keyframe_transform / ngicp_keyframe_get; k_keyframe_move in csrc/ngicp_keyframe_move.h) against the
numpy model of the definition (tests/_keyframe_move_model.py, which proves itself in test_keyframe_move_model_cpu.py).

Everything is compared with np.array_equal: the definition spells every operation (the float32 transform in PCL's order, rotate_sym in
FP64, nothing fused), min and max do not depend on the order, and the rolling-map tests already hold rotate_sym to the same model bit for
bit.  Sizes are chosen for wave and block edges (1, 63, 64, 65, 257 points; 3008 = 11 blocks and three quarters), not for the workload."""
import ctypes as C

import numpy as np
import pytest

import _keyframe_move_model as km
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _pose(axis, angle, t):
    T = np.eye(4)
    T[:3, :3] = _rot(axis, angle)
    T[:3, 3] = t
    return T.astype(np.float32)


def _spd(n, seed):
    A = np.random.default_rng(seed).normal(0, 0.1, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return out


def _cube(n, half, seed, offset=(0.0, 0.0, 0.0)):
    return (np.random.default_rng(seed).uniform(-half, half, (n, 3)) + np.asarray(offset)).astype(np.float32)


def _same(a, b):
    """byte for byte (array_equal would let -0.0 pass for 0.0)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_kf(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _read_store(g):
    return [g.getKeyframe(i) for i in range(g.numKeyframes())]


def _add(g, prod, pts, covs=None):
    """a keyframe through addKeyframe: the producer's source with the covariances given (tiny clouds) or computed (k = 20, PLANE)"""
    prod.setInputSource(pts)
    if covs is None:
        prod.calculateSourceCovariances()
    else:
        prod.setSourceCovariances(covs)
    return g.addKeyframe(prod)


def _dlo_pair(ng):
    s2s, s2m = ng.NanoGICP(), ng.NanoGICP()
    for e, k, d in ((s2s, 10, 1.0), (s2m, 20, 0.5)):
        e.setCorrespondenceRandomness(k); e.setMaxCorrespondenceDistance(d); e.setMaximumIterations(32); e.setTransformationEpsilon(0.01)
    return s2s, s2m


# ---------------------------------------------------------------------------------------------------------------- 1. reading a keyframe back
def test_get_keyframe_after_each_add_route(ng):
    prod, g = ng.NanoGICP(), ng.NanoGICP()
    scan = _cube(2500, 20.0, 1)
    T = clouds.make_pose((1.0, -0.5, 0.2), (1.0, -2.0, 30.0)).astype(np.float32)
    prod.setInputSource(scan)
    prod.calculateSourceCovariances()
    a = g.addKeyframe(prod)
    pa, ca = g.getKeyframe(a)
    assert pa.dtype == np.float32 and pa.shape == (2500, 3) and ca.shape == (2500, 4, 4)
    assert np.array_equal(pa, scan) and np.array_equal(ca, prod.getSourceCovariances())
    b = g.addKeyframeTransformed(prod, T)
    assert np.array_equal(g.getKeyframe(b)[0], prod.transformSource(T))
    c = g.addKeyframeTransformedFiltered(prod, T, 1.5)
    assert 0 < g.keyframeSize(c) < 2500
    for kid in (a, b, c):
        pts, covs = g.getKeyframe(kid)
        g.setSubmapKeyframes([kid])
        assert np.array_equal(g.targetPoints(), pts) and np.array_equal(g.getTargetCovariances(), covs)
        assert len(pts) == g.keyframeSize(kid)
        assert not covs[:, 3, :].any() and not covs[:, :, 3].any()
    # either array alone, a stride, the errors
    n = C.c_size_t(0)
    wide = np.full((2500, 4), 7.0, np.float32)
    assert g._L.ngicp_keyframe_get(g._h, a, wide.ctypes.data_as(C.POINTER(C.c_float)), 16, None, C.byref(n)) == 0 and n.value == 2500
    assert np.array_equal(wide[:, :3], scan) and (wide[:, 3] == 7.0).all()
    c16 = np.empty((2500, 16))
    assert g._L.ngicp_keyframe_get(g._h, a, None, 0, c16.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    assert np.array_equal(c16.reshape(-1, 4, 4).transpose(0, 2, 1), ca)
    for kid, stride in ((3, 12), (-1, 12), (a, 8), (a, 14)):
        assert g._L.ngicp_keyframe_get(g._h, kid, wide.ctypes.data_as(C.POINTER(C.c_float)), stride, None, None) == -2  # NGICP_ERR_ARG
    prod.close(); g.close()


# ---------------------------------------------------------------------------------------------------------------- 2. one call, many keyframes
SIZES = (300, 1, 63, 500, 64, 65, 257, 3008)   # ids 0..7; 0 and 3 are not moved
MOVED = (7, 1, 5, 2, 6, 4)                     # out of order


def _move_poses():
    return np.stack([
        _pose([1, 2, 3], 0.7, [3, -2, 1]),            # 3008 points
        _pose([-1, 0.3, 2], 2.1, [300, -5, 12]),      # 1 point, 300 m away
        np.eye(4, dtype=np.float32),                  # 65: the identity
        _pose([0.2, -1, 0.4], -1.3, [-7, 0.5, 2]),    # 63
        _pose([3, 1, -2], 3.0, [0.25, 40, -3]),       # 257
        _pose([0, 1, 1], 0.01, [0.3, -0.1, 0.05]),    # 64: a loop closure's small correction
    ])


@pytest.fixture(scope="module")
def big_store(ng):
    prod, g = ng.NanoGICP(), ng.NanoGICP()
    for i, n in enumerate(SIZES):
        pts = _cube(n, 15.0, 100 + i, offset=(5.0 * i, -3.0 * i, 0.5 * i))
        _add(g, prod, pts, _spd(n, 200 + i) if n < 100 else None)
    before = _read_store(g)
    stale = g.transformKeyframes(MOVED, _move_poses())
    yield g, before, stale
    prod.close(); g.close()


def test_one_call_moves_many_keyframes_and_equals_the_model(big_store):
    g, before, stale = big_store
    assert stale is False  # no submap was ever set
    want = km.move(before, MOVED, _move_poses())
    got = _read_store(g)
    for i, n in enumerate(SIZES):
        assert got[i][0].shape == (n, 3) and g.keyframeSize(i) == n
        assert np.array_equal(got[i][0], want[i][0]), f"points of keyframe {i} ({n} points)"
        assert np.array_equal(got[i][1], want[i][1]), f"covariances of keyframe {i} ({n} points)"
    for i in (0, 3):  # not listed: the same bytes
        assert _same(got[i][0], before[i][0]) and _same(got[i][1], before[i][1])
    assert _same(got[5][0], before[5][0]) and np.array_equal(got[5][1], before[5][1])  # the identity
    assert not np.array_equal(got[7][0], before[7][0])
    assert g.keyframeTransformKernelMs() > 0.0


def test_moved_keyframes_assemble_into_the_submap_of_the_models_clouds(big_store):
    """the box a move leaves is the one the submap's index is built in: every point of every moved keyframe comes back in place"""
    g, before, _ = big_store
    want = km.move(before, MOVED, _move_poses())
    ids = [7, 0, 1, 6, 2]
    assert g.setSubmapKeyframes(ids) is True
    assert np.array_equal(g.targetPoints(), np.concatenate([want[i][0] for i in ids]))
    assert np.array_equal(g.getTargetCovariances(), np.concatenate([want[i][1] for i in ids]))


# ---------------------------------------------------------------------------------------------------------------- 3. copy on move
def test_a_move_leaves_the_producer_that_shares_the_buffers_alone(ng):
    prod, g = ng.NanoGICP(), ng.NanoGICP()
    pts, tgt = _cube(3000, 10.0, 5), _cube(3000, 10.0, 5) + np.float32(0.05)
    prod.setInputSource(pts)
    prod.setInputTarget(tgt)
    prod.calculateSourceCovariances()
    kid = g.addKeyframe(prod)  # adopts the producer's cloud and covariance buffers, no copy

    def producer_state():
        prod.align()
        return (prod.transformSource(np.eye(4)), prod.getSourceCovariances(), prod.getFinalTransformation().copy(), prod.nr_iterations_,
                prod.getFinalHessian().copy())

    s0 = producer_state()
    kf0 = g.getKeyframe(kid)
    T = _pose([1, 1, 0], 0.5, [10, 0, -1])
    g.transformKeyframes([kid], T[None])
    s1 = producer_state()
    assert all(np.array_equal(x, y) for x, y in zip(s0, s1))
    assert _same_kf(g.getKeyframe(kid), km.move([kf0], [0], T[None])[0])
    prod.close(); g.close()


# ---------------------------------------------------------------------------------------------------------------- 4. / 5. the target and the submap
def _result(e):
    return (e.getFinalTransformation().copy(), e.nr_iterations_, e.converged_, e.getFinalHessian().copy())


def _same_result(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("voxel", [False, True], ids=["exact", "voxel-merged"])
def test_moving_a_keyframe_of_the_submap(ng, voxel):
    w = clouds.scan_to_submap(6_000, 4)
    kfs = np.split(w.target, np.cumsum(w.keyframe_sizes)[:-1])
    s2s, s2m = _dlo_pair(ng)
    ref_prod, ref = _dlo_pair(ng)
    for e in (s2m, ref):
        if voxel:
            e.setVoxelResolution(1.0)
            e.setVoxelSubmapMerge(True)
    for kf in kfs:
        s2s.setInputSource(kf); s2s.calculateSourceCovariances()
        s2m.addKeyframe(s2s)
    a, b, c, d = 0, 1, 2, 3
    s2m.setInputSource(w.source)
    assert s2m.setSubmapKeyframes([a, b, c]) is True

    def target_state():
        s2m.align(w.guess)
        st = [s2m.targetPoints(), s2m.getTargetCovariances(), *_result(s2m)]
        if voxel:
            st += list(s2m.voxelMap())
        return st

    before = _read_store(s2m)
    t0 = target_state()
    builds0 = s2m.voxelMapBuilds() if voxel else 0
    # a keyframe outside the submap: the memo stays
    T_d = _pose([0, 0, 1], 0.02, [0.2, 0.1, 0.0])
    assert s2m.transformKeyframes([d], T_d[None]) is False
    assert s2m.setSubmapKeyframes([a, b, c]) is False
    # a keyframe of the submap: the target is not touched, the memo is forgotten
    T_b = _pose([0.1, -0.2, 1], 0.015, [0.12, -0.08, 0.03])
    assert s2m.transformKeyframes([b], T_b[None]) is True
    t1 = target_state()
    assert all(np.array_equal(x, y) for x, y in zip(t0, t1))
    if voxel:
        assert s2m.voxelMapBuilds() == builds0  # the map of the unchanged target stands
    assert s2m.setSubmapKeyframes([a, b, c]) is True
    assert s2m.setSubmapKeyframes([a, b, c]) is False
    # the same store built the host way from the model's outputs
    want = km.move(km.move(before, [d], T_d[None]), [b], T_b[None])
    for i, (p, cov) in enumerate(want):
        assert _same_kf(s2m.getKeyframe(i), (p, cov))
        ref_prod.setInputSource(p); ref_prod.setSourceCovariances(cov)
        ref.addKeyframe(ref_prod)
    ref.setInputSource(w.source)
    assert ref.setSubmapKeyframes([a, b, c]) is True
    assert np.array_equal(s2m.targetPoints(), ref.targetPoints()) and np.array_equal(s2m.getTargetCovariances(), ref.getTargetCovariances())
    assert np.array_equal(s2m.targetPoints(), np.concatenate([want[i][0] for i in (a, b, c)]))
    if voxel:
        for x, y in zip(s2m.keyframeVoxelMap(b), ref.keyframeVoxelMap(b)):
            assert np.array_equal(x, y)
    s2m.align(w.guess); ref.align(w.guess)
    assert _same_result(_result(s2m), _result(ref))
    if voxel:
        for x, y in zip(s2m.voxelMap(), ref.voxelMap()):
            assert np.array_equal(x, y)
        assert s2m.voxelMapMergeStats()["merged_builds"] == 2 and ref.voxelMapMergeStats()["merged_builds"] == 1  # both by the merged route
    assert not _same_result(_result(s2m), tuple(t0[2:6]))  # (the move was not a no-op for the alignment)
    for e in (s2s, s2m, ref_prod, ref):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 6. twice
def test_two_moves_are_the_model_applied_twice(ng):
    prod, g = ng.NanoGICP(), ng.NanoGICP()
    kid = _add(g, prod, _cube(700, 30.0, 9))
    kf0 = g.getKeyframe(kid)
    A, B = _pose([1, 2, 3], 0.7, [3, -2, 1]), _pose([0, 1, -1], -0.4, [-7, 0.5, 2])
    g.transformKeyframes([kid], A[None])
    g.transformKeyframes([kid], B[None])
    twice = km.move(km.move([kf0], [0], A[None]), [0], B[None])[0]
    once = km.move([kf0], [0], (B.astype(np.float64) @ A.astype(np.float64)).astype(np.float32)[None])[0]
    got = g.getKeyframe(kid)
    assert _same_kf(got, twice) and not np.array_equal(got[0], once[0])
    prod.close(); g.close()


# ---------------------------------------------------------------------------------------------------------------- 7. all or nothing
def test_every_refusal_changes_nothing(ng):
    prod, g = ng.NanoGICP(), ng.NanoGICP()
    g.setVoxelResolution(1.0)
    g.setVoxelSubmapMerge(True)
    _add(g, prod, np.array([[2.0, 0.0, 0.0], [1.0, 1.0, 1.0], [-1.0, 0.5, 0.25]], np.float32), _spd(3, 1))
    _add(g, prod, _cube(200, 5.0, 2))
    _add(g, prod, _cube(65, 5.0, 3), _spd(65, 4))
    ids = [0, 1, 2]
    g.setInputSource(_cube(100, 5.0, 6))
    assert g.setSubmapKeyframes(ids) is True
    g.align()
    keep = _read_store(g)
    parts = [g.keyframeVoxelMap(i) for i in ids]
    target = [g.targetPoints(), g.getTargetCovariances(), *g.voxelMap(), *_result(g)]
    parts_built = g.voxelMapMergeStats()

    eye = np.eye(4, dtype=np.float32)
    bad_nan, bad_inf, bad_row, bad_w, big = (eye.copy() for _ in range(5))
    bad_nan[1, 2] = np.nan
    bad_inf[0, 3] = np.inf
    bad_row[3, 0] = 1e-30
    bad_w[3, 3] = 2
    big[0, 0] = 3e38  # finite, and 3e38 * 2 is not: found on the device
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int)
    one_id = np.array([1], np.int32)
    flat = np.ascontiguousarray(eye.T).reshape(-1)
    raw = [
        lambda: g._L.ngicp_keyframe_transform(g._h, None, 1, flat.ctypes.data_as(f32p), None),
        lambda: g._L.ngicp_keyframe_transform(g._h, one_id.ctypes.data_as(i32p), 1, None, None),
        lambda: g._L.ngicp_keyframe_transform(g._h, one_id.ctypes.data_as(i32p), 0, flat.ctypes.data_as(f32p), None),
    ]
    cases = [
        ([3], eye[None], "unknown keyframe"), ([-1], eye[None], "unknown keyframe"),
        ([1, 2, 1], np.stack([eye] * 3), "positions 0 and 2"),
        ([1], bad_nan[None], "not finite"), ([2, 1], np.stack([eye, bad_inf]), "not finite"),
        ([1], bad_row[None], "last row"), ([1], bad_w[None], "last row"),
        ([1, 0, 2], np.stack([_pose([0, 0, 1], 0.3, [1, 2, 3]), big, eye]), "moved coordinate"),
    ]

    def unchanged():
        now = _read_store(g)
        assert all(_same(x[0], y[0]) and _same(x[1], y[1]) for x, y in zip(now, keep))
        assert g.setSubmapKeyframes(ids) is False
        assert g.voxelMapMergeStats() == parts_built  # no voxel part was dropped and rebuilt
        for i in ids:
            assert all(np.array_equal(x, y) for x, y in zip(g.keyframeVoxelMap(i), parts[i]))
        assert all(np.array_equal(x, y) for x, y in zip([g.targetPoints(), g.getTargetCovariances(), *g.voxelMap(), *_result(g)], target))

    for call in raw:
        assert call() == -2  # NGICP_ERR_ARG
        unchanged()
    for kf_ids, Ts, text in cases:
        with pytest.raises(ng.NgicpError, match=text) as err:
            g.transformKeyframes(kf_ids, Ts)
        assert err.value.code == -2
        unchanged()
    # and the store still moves
    assert g.transformKeyframes([1], _pose([0, 0, 1], 0.3, [1, 2, 3])[None]) is True
    assert _same_kf(g.getKeyframe(1), km.move(keep, [1], _pose([0, 0, 1], 0.3, [1, 2, 3])[None])[1])
    prod.close(); g.close()
