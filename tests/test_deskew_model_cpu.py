"""tests/_deskew_model.py (the deskew definition of include/ngicp.h in numpy float64, in the engine's operation order) against an
independent statement: scipy's Slerp over the ABSOLUTE poses - the same geodesic R_k exp(alpha log(R_k^T R_{k+1})) - with linear
translation, moved into the reference frame afterwards.  And clouds.skew_scan, the inverse operation, against the model."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation, Slerp

import _deskew_model as dm
from _deskew_cases import random_trajectory, times_for
from direct_lidar_odometry_amd import clouds


@pytest.mark.parametrize("M", [2, 3, 40])
@pytest.mark.parametrize("with_ref", [False, True], ids=["identity-ref", "ref"])
def test_model_matches_slerp_and_linear_translation(M, with_ref):
    tau, poses = random_trajectory(M, 10 + M)
    T_ref = clouds.make_pose((1.5, -0.7, 0.3), (4.0, -7.0, 25.0)) if with_ref else None
    rng = np.random.default_rng(20 + M)
    n = 400
    p = (rng.uniform(-1, 1, (n, 3)) * (40.0, 40.0, 5.0)).astype(np.float32)
    s = times_for(tau, n, 30 + M)
    got = dm.deskew_f64(p, s, tau, poses, T_ref)

    sc = np.clip(s, tau[0], tau[-1])  # no extrapolation
    R = Slerp(tau, Rotation.from_matrix(poses[:, :3, :3]))(sc).as_matrix()
    t = np.stack([np.interp(sc, tau, poses[:, i, 3]) for i in range(3)], axis=-1)
    world = np.einsum("nij,nj->ni", R, p.astype(np.float64)) + t
    Tr = np.eye(4) if T_ref is None else T_ref
    ref = (world - Tr[:3, 3]) @ Tr[:3, :3]  # R_ref^T (x - t_ref)

    tol = 1e-12 * (1.0 + np.linalg.norm(p.astype(np.float64), axis=1) + max(np.abs(poses[:, :3, 3]).max(), dm.max_abs_t(tau, poses, T_ref)))
    err = np.abs(got - ref).max(axis=1)
    print(f"M = {M}: max err {err.max():.3e}, min tolerance {tol.min():.3e}")
    assert (err <= tol).all()


def test_model_holds_the_end_poses_and_hits_the_knots():
    tau, poses = random_trajectory(3, 5)
    p = np.array([[1.0, 2.0, 3.0]], np.float32)
    for s, k in ((tau[0] - 1.0, 0), (tau[0], 0), (tau[1], 1), (tau[2], 2), (tau[2] + 1.0, 2)):
        got = dm.deskew_f64(p, np.array([s]), tau, poses)[0]
        want = poses[k, :3, :3] @ p[0].astype(np.float64) + poses[k, :3, 3]
        assert np.abs(got - want).max() <= 1e-12 * (1 + np.abs(want).max()), (s, k)


def test_model_edge_cases():
    tau, poses = random_trajectory(3, 6)
    p = np.array([[1, 2, 3], [np.nan, 2, 3], [1, np.inf, 3], [4, 5, 6], [7, 8, 9]], np.float32)
    s = np.array([0.01, 0.01, np.nan, np.nan, np.inf])
    out = dm.deskew(p, s, tau, poses)
    assert np.isfinite(out[0]).all() and not np.array_equal(out[0], p[0])
    assert np.array_equal(out[1:3].view(np.uint32), p[1:3].view(np.uint32))  # non-finite points: copied
    assert np.isnan(out[3:]).all()                                           # finite points without a finite time: NaN


def test_time_formats_are_two_roundings():
    raw = np.array([0, 1, 99_999_999, 4_294_967_295], np.uint32)
    assert np.array_equal(dm.seconds(raw, dm.TIME_U32_NS, 17.25), raw.astype(np.float64) * 1e-9 + 17.25)
    f = np.array([0.1, 0.033333], np.float32)
    assert np.array_equal(dm.seconds(f, dm.TIME_F32_S), f.astype(np.float64))
    assert np.array_equal(dm.seconds(f, dm.TIME_F32_S), dm.seconds(f.astype(np.float64), dm.TIME_F64_S))


def roundtrip_bound(a, b) -> np.float32:
    """2 float32 ulps of the largest coordinate magnitude: skew_scan rounds once (<= 1/2 ulp per coordinate, <= sqrt(3)/2 ulp as a
    vector, which the deskew's rotation can turn into one coordinate) and the deskew rounds once more (1/2 ulp): 1.37 ulps < 2."""
    return 2 * np.spacing(np.float32(max(np.abs(a).max(), np.abs(b).max())))


@pytest.mark.parametrize("M", [2, 40])
def test_skew_scan_then_model_returns_the_cloud(M):
    w = clouds.scan_to_submap(3008, n_keyframes=1)
    scan = w.source
    tau, poses = random_trajectory(M, 40 + M, max_rot=0.1 if M == 2 else 0.02)
    T_ref = poses[-1]
    s = clouds.sweep_times(len(scan), sweep_s=tau[-1] - tau[0], t0=tau[0])
    raw = clouds.skew_scan(scan, s, tau, poses, T_ref)
    assert raw.dtype == np.float32 and np.abs(raw - scan).max() > 0.01  # it does distort
    back = dm.deskew(raw, s, tau, poses, T_ref)
    bound = roundtrip_bound(scan, raw)
    err = np.abs(back.astype(np.float64) - scan.astype(np.float64)).max()
    print(f"M = {M}: round trip max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_sweep_times_follow_the_azimuth_columns():
    s = clouds.sweep_times(3008, rings=16, sweep_s=0.1, t0=2.0)
    assert s.dtype == np.float64 and s[0] == 2.0 and (np.diff(s) >= 0).all() and s[-1] < 2.1
    assert (s.reshape(-1, 16) == s[::16, None]).all() and len(np.unique(s)) == 188
