"""The numpy model of moving keyframes (tests/_keyframe_move_model.py) holds to its definition (include/ngicp.h "moving keyframes").
The engine is held to the model, bit for bit, in test_gpu_keyframe_move.py."""
import numpy as np
import pytest

import _keyframe_move_model as km


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


def _spd(rng, n):
    A = rng.normal(size=(n, 3, 3))
    C = np.zeros((n, 4, 4))
    C[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return C


@pytest.fixture(scope="module")
def store():
    rng = np.random.default_rng(11)
    return [(rng.uniform(-40, 40, (n, 3)).astype(np.float32), _spd(rng, n)) for n in (1, 5, 64, 130)]


def test_identity_returns_the_input(store):
    out = km.move(store, [2, 0], np.stack([np.eye(4, dtype=np.float32)] * 2))
    for (p, c), (q, d) in zip(store, out):
        assert np.array_equal(p, q) and np.array_equal(c, d)


def test_covariances_stay_symmetric_keep_the_zero_frame_and_their_eigenvalues(store):
    T = _pose([1, 2, 3], 0.7, [3, -2, 1])
    _, c = km.move_one(*store[3], T)
    assert np.array_equal(c, c.transpose(0, 2, 1))
    assert not c[:, 3, :].any() and not c[:, :, 3].any()
    # an orthonormal R: the float32 entries are 6e-8 off an exact rotation, so the test rotates by the DOUBLE matrix it checks against
    R = _rot([1, 2, 3], 0.7)
    for C in store[3][1][:40]:
        w0 = np.linalg.eigvalsh(C[:3, :3])
        w1 = np.linalg.eigvalsh(km.rotate_sym(R, C[:3, :3]))
        assert np.allclose(w1, w0, rtol=1e-12, atol=0)


def _exact(T, p):
    T64, p64 = np.asarray(T, np.float32).astype(np.float64), p.astype(np.float64)
    return p64 @ T64[:3, :3].T + T64[:3, 3]


def test_points_agree_with_a_float64_product_to_one_ulp_at_the_coordinates_magnitude(store):
    """Where the 3x3 block holds only 0 and +-1 (a translation, an axis permutation with sign flips) every product is exact and so is a sum
    with 0: one addition rounds, and the result is within half an ulp of float32 AT ITS OWN MAGNITUDE of the float64 product.  Held to the
    1 ulp the definition is stated with."""
    perm = np.array([[0, -1, 0, 300], [0, 0, 1, -5], [-1, 0, 0, 12], [0, 0, 0, 1]], np.float32)
    shift = np.eye(4, dtype=np.float32)
    shift[:3, 3] = [300, -0.125, 1e-3]
    p = store[3][0]
    for T in (perm, shift):
        q, _ = km.move_one(p, store[3][1], T)
        assert q.dtype == np.float32
        exact = _exact(T, p)
        err = np.abs(q.astype(np.float64) - exact)
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        print(f"largest error {(err / ulp).max():.3f} ulp at the coordinate's own magnitude")
        assert (err <= ulp).all()


def test_points_under_a_general_pose_stay_within_the_roundings_of_the_stated_order(store):
    """A general rotation: three products and three sums, each rounded to float32 (half an ulp of a value that is at most
    mag = |x m0| + |y m1| + |z m2| + |t|), so the result is within 6 * 0.5 = 3 ulp of float32 at mag of the float64 product; measured
    1.3 (both poses).  No bound at the result's own magnitude exists here: where the terms cancel the same error is 47 and 85 ulp of the
    small result."""
    p = store[3][0]
    for T in (_pose([-1, 0.3, 2], 2.1, [300, -5, 12]), _pose([1, 2, 3], 0.7, [3, -2, 1])):
        q, _ = km.move_one(p, store[3][1], T)
        exact = _exact(T, p)
        T64 = T.astype(np.float64)
        mag = np.abs(p.astype(np.float64)) @ np.abs(T64[:3, :3]).T + np.abs(T64[:3, 3])
        err = np.abs(q.astype(np.float64) - exact)
        print(f"largest error {(err / np.spacing(mag.astype(np.float32))).max():.3f} ulp at the magnitude of the terms")
        assert (err <= 3 * np.spacing(mag.astype(np.float32)).astype(np.float64)).all()


def test_only_the_listed_keyframes_change_and_the_input_is_never_written(store):
    before = [(p.copy(), c.copy()) for p, c in store]
    T = np.stack([_pose([0, 0, 1], 0.3, [1, 2, 3]), _pose([1, 1, 0], -1.0, [0, 0, 9])])
    out = km.move(store, [3, 1], T)
    for i in (0, 2):
        assert out[i][0] is store[i][0] and out[i][1] is store[i][1]
    for j, i in enumerate((3, 1)):
        q, c = km.move_one(*store[i], T[j])
        assert np.array_equal(out[i][0], q) and np.array_equal(out[i][1], c)
        assert not np.array_equal(out[i][0], store[i][0])
    for (p, c), (p0, c0) in zip(store, before):
        assert np.array_equal(p, p0) and np.array_equal(c, c0)


def test_two_moves_are_two_roundings_not_the_composition(store):
    A, B = _pose([1, 2, 3], 0.7, [3, -2, 1]), _pose([0, 1, -1], -0.4, [-7, 0.5, 2])
    twice = km.move(km.move(store, [3], A[None]), [3], B[None])[3]
    once = km.move(store, [3], (B.astype(np.float64) @ A.astype(np.float64)).astype(np.float32)[None])[3]
    assert np.allclose(twice[0], once[0], atol=1e-3) and not np.array_equal(twice[0], once[0])


def test_box_is_the_exact_min_and_max(store):
    q, _ = km.move_one(*store[2], _pose([1, 0, 0], 1.0, [0, 0, 0]))
    lo, hi = km.box(q)
    assert lo.dtype == np.float32 and (q >= lo).all() and (q <= hi).all()
    assert all(lo[d] in q[:, d] and hi[d] in q[:, d] for d in range(3))


def test_every_refusal_leaves_the_store_alone(store):
    eye = np.eye(4, dtype=np.float32)
    bad_nan, bad_inf, bad_row, bad_w, big = (eye.copy() for _ in range(5))
    bad_nan[1, 2] = np.nan
    bad_inf[0, 3] = np.inf
    bad_row[3, 0] = 1e-30
    bad_w[3, 3] = 2
    big[0, 0] = 3e38  # finite, and 3e38 * 2 is not
    cases = [
        (None, eye[None]), ([0], None), ([], np.zeros((0, 4, 4), np.float32)),
        ([4], eye[None]), ([-1], eye[None]),
        ([1, 2, 1], np.stack([eye] * 3)),
        ([0], bad_nan[None]), ([0], bad_inf[None]), ([0], bad_row[None]), ([0], bad_w[None]),
        ([1, 0], np.stack([eye, big])),
    ]
    st = [(p.copy(), c.copy()) for p, c in store]
    st[0] = (np.array([[2, 0, 0]], np.float32), st[0][1])
    keep = [(p.copy(), c.copy()) for p, c in st]
    for ids, Ts in cases:
        with pytest.raises(km.Refused):
            km.move(st, ids, Ts)
        for (p, c), (p0, c0) in zip(st, keep):
            assert np.array_equal(p, p0) and np.array_equal(c, c0)
    with pytest.raises(km.Refused, match="positions 0 and 2"):
        km.move(st, [1, 2, 1], np.stack([eye] * 3))
