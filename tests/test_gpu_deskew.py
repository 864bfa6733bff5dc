"""GPU tests (-m gpu) of the motion deskew (csrc/ngicp_deskew.h: k_deskew_prepare, k_deskew_unpack) and of the ABI around it
(ngicp_deskew_cloud, ngicp_preprocess_scan_deskewed), against the numpy float64 restatement tests/_deskew_model.py, which
test_deskew_model_cpu.py proves against scipy's Slerp.

Tolerance of the comparison with the model, per output coordinate:
    |float64(out) - model_f64| <= 0.5 * spacing(float32(|model_f64|)) + 1e-12 * (1 + |p| + max|t'|)
The first term is the engine's single rounding to float32; the second the float64 evaluation difference between the device's and the
host's libm (sin, cos, atan2, sqrt) carried through ~60 operations on values of size |p| + |t'|.  Everything else is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _deskew_cases as dc
import _deskew_model as dm
import _filter_cases as fc
import _filter_model as fmodel
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -2, -3  # include/ngicp.h
c_f32p = C.POINTER(C.c_float)
T_REF = clouds.make_pose((1.5, -0.7, 0.3), (4.0, -7.0, 25.0))


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture(scope="module")
def g(ng):
    return ng.NanoGICP()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_raw(seconds, fmt):
    """Float64 seconds -> the nearest raw values of a time format (the engine adds time_offset to them afterwards)."""
    s = np.asarray(seconds, np.float64)
    return np.round(s * 1e9).astype(np.uint32) if fmt == dm.TIME_U32_NS else s.astype(dm.DTYPE[fmt])


def points(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 3)) * (40.0, 40.0, 5.0)).astype(np.float32)


def check_against_model(out, p, s, tau, poses, T_ref, what):
    model = dm.deskew_f64(p, s, tau, poses, T_ref)
    tol = 0.5 * np.spacing(np.abs(model).astype(np.float32)).astype(np.float64) + \
        1e-12 * (1.0 + np.linalg.norm(p.astype(np.float64), axis=1) + dm.max_abs_t(tau, poses, T_ref))[:, None]
    err = np.abs(out.astype(np.float64) - model)
    worst = float((err / tol).max())
    print(f"{what}: worst |out - model| / tolerance = {worst:.3f}, max err {err.max():.3e}")
    assert out.dtype == np.float32 and out.shape == model.shape
    assert (err <= tol).all(), what


# ------------------------------------------------------------------ 1. against the model
# (time format, where the time lies: None = an array of its own, else (point stride, byte offset inside the record), time_offset)
LAYOUTS = [(dm.TIME_F32_S, None, 0.0), (dm.TIME_F64_S, None, 0.0), (dm.TIME_U32_NS, None, 17.25), (dm.TIME_F32_S, (24, 12), 0.0),
           (dm.TIME_F64_S, (32, 16), -3.5), (dm.TIME_U32_NS, (48, 44), 0.0), (dm.TIME_F64_S, (24, 16), 0.0), (dm.TIME_F32_S, (32, 28), 0.25)]


@pytest.mark.parametrize("M", [2, 3, 40, 256])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_matches_the_model(g, n, M):
    """Every knot exactly, one time below tau_0 and one above tau_{M-1} are among the times (as far as n reaches); they are shuffled, so
    a wave's lanes search unrelated segments."""
    ideal_tau, poses = dc.random_trajectory(M, 100 + M, max_rot=0.5 if M <= 40 else 0.2, t0=0.02)
    ideal_s = dc.times_for(ideal_tau, n, 200 + n + M)
    p = points(n, 300 + n)
    for fmt, where, offset in LAYOUTS:
        raw_tau, raw_s = to_raw(ideal_tau, fmt), to_raw(ideal_s, fmt)
        tau, s = dm.seconds(raw_tau, fmt, offset), dm.seconds(raw_s, fmt, offset)
        assert (np.diff(tau) > 0).all()
        if n >= M + 2:
            assert np.isin(tau, s).all() and s.min() < tau[0] and s.max() > tau[-1]
        T_ref = None if (fmt, where) == (dm.TIME_F64_S, None) else T_REF
        if where is None:
            holder = np.zeros(2 * n, raw_s.dtype)
            holder[::2] = raw_s
            times = holder[::2] if fmt == dm.TIME_F32_S else raw_s  # once through a strided view
            out = g.deskewCloud(p, times, tau, poses, T_ref, time_offset=offset)
        else:
            stride, off = where
            rec = dc.records(p, stride, raw_s, off)
            out = g.deskewCloud(rec, off // 4, tau, poses, T_ref, time_format=fmt, time_offset=offset)
        check_against_model(out, p, s, tau, poses, T_ref, f"n {n} M {M} format {fmt} at {where}")


# ------------------------------------------------------------------ 2. exact anchors
def test_identity_trajectory_returns_the_input_bits(g):
    p = points(5000, 1)
    assert not (bits(p) == 0x80000000).any()  # (-0.0 would come back as +0.0: include/ngicp.h)
    s = dc.times_for(np.array([0.0, 0.05, 0.1]), len(p), 2)
    out = g.deskewCloud(p, s, [0.0, 0.05, 0.1], np.tile(np.eye(4), (3, 1, 1)))
    assert np.array_equal(bits(out), bits(p))


def test_nonfinite_points_are_copied_and_nonfinite_times_give_nan(g):
    tau, poses = dc.random_trajectory(3, 7)
    cloud = fc.scan_cloud(2000, 8)[:, :5].copy()  # x y z 1 intensity; about 1 % rows with a NaN / Inf coordinate
    bad_p = ~np.isfinite(cloud[:, :3]).all(axis=1)
    assert bad_p.sum() >= 10
    s = dc.times_for(tau, len(cloud), 9).astype(np.float32)
    bad_s = np.zeros(len(cloud), bool)
    bad_s[[0, 64, 65, 1999]] = True
    bad_s[np.flatnonzero(bad_p)[:2]] = True  # a non-finite point with a non-finite time is still copied
    s[bad_s] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad_s.sum()))
    want = dm.deskew(cloud[:, :3], s.astype(np.float64), tau, poses, T_REF)
    out3 = g.deskewCloud(cloud, s, tau, poses, T_REF)
    out4 = g.preprocessScanDeskewed(cloud, s, tau, poses, T_REF, remove_nan=False, intensity_col=4)
    for out in (out3, out4[:, :3]):
        assert np.array_equal(bits(out[bad_p]), bits(cloud[bad_p, :3]))
        assert (bits(out[bad_s & ~bad_p]) == 0x7FC00000).all()
        ok = ~bad_p & ~bad_s
        assert np.isfinite(out[ok]).all() and np.abs(out[ok] - want[ok]).max() < 1e-4
    assert np.array_equal(bits(out4[:, 3]), bits(cloud[:, 4]))  # intensity carried through, NaN-time rows included
    assert np.array_equal(bits(out3), bits(out4[:, :3]))
    kept = g.preprocessScanDeskewed(cloud, s, tau, poses, T_REF, remove_nan=True, intensity_col=4)
    assert np.array_equal(bits(kept), bits(out4[~bad_p & ~bad_s]))  # removeNaN drops both kinds


def test_result_does_not_depend_on_n(g):
    tau, poses = dc.random_trajectory(40, 11)
    p = points(5000, 12)
    s = dc.times_for(tau, 5000, 13)
    big = g.deskewCloud(p, s, tau, poses, T_REF)
    small = g.deskewCloud(p[:65], s[:65], tau, poses, T_REF)
    assert np.array_equal(bits(big[:65]), bits(small))


def test_time_formats_agree_on_the_same_instants(g):
    tau, poses = dc.random_trajectory(40, 14, t0=0.02)
    p = points(5000, 15)
    s = dc.times_for(tau, 5000, 16)
    f32 = s.astype(np.float32)
    a = g.deskewCloud(p, f32, tau, poses, T_REF)
    b = g.deskewCloud(p, f32.astype(np.float64), tau, poses, T_REF)
    assert np.array_equal(bits(a), bits(b))
    ns = np.round(s * 1e9).astype(np.uint32)
    c = g.deskewCloud(p, ns, tau, poses, T_REF)
    d = g.deskewCloud(p, ns.astype(np.float64) * 1e-9, tau, poses, T_REF)
    assert np.array_equal(bits(c), bits(d))
    assert not np.array_equal(bits(a), bits(c))  # (different instants: the formats are not interchangeable for free)


# ------------------------------------------------------------------ 3. route equivalence
@pytest.mark.parametrize("with_intensity", [True, False], ids=["intensity", "no-intensity"])
@pytest.mark.parametrize("stages", fc.STAGES, ids=[s[0] for s in fc.STAGES])
def test_deskewed_preprocess_equals_deskew_then_preprocess(g, stages, with_intensity):
    _, remove_nan, crop, leaf = stages
    tau, poses = dc.random_trajectory(40, 21, max_rot=0.02)
    x = fc.scan_cloud(8193, 22).copy()  # 32-byte records: x y z 1 | intensity . . .
    s = dc.times_for(tau, len(x), 23).astype(np.float32)
    s[[5, 700, 8192]] = np.nan
    x[:, 5] = s  # the time in the record's padding, byte 20
    icol = 4 if with_intensity else None
    got = g.preprocessScanDeskewed(x, 5, tau, poses, T_REF, remove_nan=remove_nan, crop_size=crop, voxel_res=leaf, intensity_col=icol)
    host = g.deskewCloud(x, 5, tau, poses, T_REF)
    want = g.preprocessScan(np.c_[host, x[:, 4]], remove_nan=remove_nan, crop_size=crop, voxel_res=leaf, intensity_col=3 if with_intensity else None)
    print(f"{stages[0]}: {len(x)} -> {len(got)} rows")
    assert 0 < len(got) and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want))


def test_deskewed_scan_becomes_the_source_without_a_download(ng):
    w = clouds.scan_to_submap(3008, 2)
    tau, poses = dc.twist_trajectory((5.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.1, 11)
    s = clouds.sweep_times(len(w.source), sweep_s=0.1)
    raw = clouds.skew_scan(w.source, s, tau, poses, poses[-1])
    a, b = ng.NanoGICP(), ng.NanoGICP()
    for e in (a, b):
        e.setMaxCorrespondenceDistance(w.max_corr_dist)
        e.setInputTarget(w.target)
    on_device = a.preprocessScanDeskewed(raw, s, tau, poses, poses[-1], remove_nan=False, set_as_source=True)  # every stage off
    host = b.deskewCloud(raw, s, tau, poses, poses[-1])
    assert np.array_equal(bits(on_device[:, :3]), bits(host))
    b.setInputSource(host)
    a.align(w.guess); b.align(w.guess)
    assert np.array_equal(bits(a.getFinalTransformation()), bits(b.getFinalTransformation()))
    assert a.nr_iterations_ == b.nr_iterations_ and a.hasConverged() == b.hasConverged()
    (ca, da), (cb, db) = a.correspondences(), b.correspondences()
    assert np.array_equal(ca, cb) and np.array_equal(bits(da), bits(db))
    assert np.array_equal(a.getSourceCovariances(), b.getSourceCovariances())


# ------------------------------------------------------------------ 4. arguments
def _desc(ng, n, **over):
    """A valid description of n points (F32 times in an array of their own, 3 poses, a reference) with fields replaced."""
    tau, poses = dc.random_trajectory(3, 31)
    kw = dict(times=np.linspace(0, 0.1, n).astype(np.float32), pose_times=tau, poses=poses, T_ref=T_REF, time_format=None, time_offset=0.0)
    kw.update(over)
    return ng.NanoGICP._deskew_desc(n, kw["times"], kw["pose_times"], kw["poses"], kw["T_ref"], kw["time_format"], kw["time_offset"])


def _call_both(g, cloud, d):
    """Both entries through the C ABI itself -> ((rc, message) of ngicp_deskew_cloud, (rc, message, n_out) of the preprocess entry)."""
    n = len(cloud)
    out3, out4, m = np.empty((max(n, 1), 3), np.float32), np.empty((max(n, 1), 4), np.float32), C.c_size_t(12345)
    dp = C.byref(d) if d is not None else None
    rc1 = g._L.ngicp_deskew_cloud(g._h, cloud.ctypes.data_as(c_f32p), n, cloud.strides[0], dp, out3.ctypes.data_as(c_f32p), 12)
    msg1 = (g._L.ngicp_last_error(g._h) or b"").decode()
    rc2 = g._L.ngicp_preprocess_scan_deskewed(g._h, cloud.ctypes.data_as(c_f32p), n, cloud.strides[0], 16, dp, 1, 1.0, 0.25, out4.ctypes.data_as(c_f32p), n,
                                              C.byref(m))
    msg2 = (g._L.ngicp_last_error(g._h) or b"").decode()
    return (rc1, msg1), (rc2, msg2, m.value)


def _bad_descriptions(ng, n):
    tau, poses = dc.random_trajectory(3, 31)
    tau257, poses257 = dc.random_trajectory(257, 32, max_rot=0.05)

    def pose_with(k, r, c, v):
        q = poses.copy()
        q[k, r, c] = v
        return q
    bad_ref = T_REF.copy(); bad_ref[3, 3] = 2.0
    nan_ref = T_REF.copy(); nan_ref[1, 3] = np.nan
    f64 = np.linspace(0, 0.1, n)
    return [
        ("n_poses", dict(pose_times=tau[:1], poses=poses[:1])),
        ("n_poses", dict(pose_times=tau257, poses=poses257)),
        ("pose_times", dict(pose_times=np.array([0.0, np.nan, 0.1]))),
        ("pose_times", dict(pose_times=np.array([0.0, np.inf, np.inf]))),
        ("pose_times", dict(pose_times=np.array([0.0, 0.05, 0.05]))),
        ("pose_times", dict(pose_times=np.array([0.0, 0.06, 0.05]))),
        ("poses_colmajor", dict(poses=pose_with(1, 0, 3, np.inf))),
        ("poses_colmajor", dict(poses=pose_with(2, 1, 1, np.nan))),
        ("poses_colmajor", dict(poses=pose_with(0, 3, 0, 1e-3))),
        ("poses_colmajor", dict(poses=pose_with(2, 3, 3, 0.0))),
        ("T_ref_colmajor", dict(T_ref=bad_ref)),
        ("T_ref_colmajor", dict(T_ref=nan_ref)),
        ("time_format", dict(time_format=3)),
        ("time_format", dict(time_format=-1)),
        ("time_offset_bytes", dict(times=8, time_format=dm.TIME_F32_S)),    # byte 32: past the 32-byte record
        ("time_offset_bytes", dict(times=7, time_format=dm.TIME_F64_S)),    # byte 28: 8 bytes do not fit, nor is it 8-aligned
        ("time_offset_bytes", dict(times=5, time_format=dm.TIME_F64_S)),    # byte 20: fits, not 8-aligned
        ("time_offset_bytes", dict(times=-1, time_format=dm.TIME_U32_NS)),
        ("time_stride_bytes", dict(times=f64, time_format=dm.TIME_F32_S, _stride=2)),
        ("time_stride_bytes", dict(times=f64, time_format=dm.TIME_F64_S, _stride=12)),
        ("time_stride_bytes", dict(times=f64, time_format=dm.TIME_U32_NS, _stride=0)),
    ]


def test_refused_arguments_leave_the_handle_usable_and_nothing_pending(ng):
    g = ng.NanoGICP()
    cloud = fc.scan_cloud(257, 33)
    valid, keep_valid = _desc(ng, len(cloud))
    cases = [("d", None)]
    keep = []
    for field, over in _bad_descriptions(ng, len(cloud)):
        stride = over.pop("_stride", None)
        d, k = _desc(ng, len(cloud), **over)
        if stride is not None:
            d.time_stride_bytes = stride
        keep.append(k)
        cases.append((field, d))
    for field, d in cases:
        g.preprocessScan(cloud, True, 1.0, 0.25, intensity_col=4)  # a preprocessed cloud is pending ...
        (rc1, msg1), (rc2, msg2, m) = _call_both(g, cloud, d)
        assert rc1 == ERR_ARG and field in msg1, (field, rc1, msg1)
        assert rc2 == ERR_ARG and field in msg2 and m == 0, (field, rc2, msg2, m)
        assert g._L.ngicp_set_source_preprocessed(g._h, 0) == ERR_STATE, field  # ... and is gone after the refused call
    # an in-record F64 time needs a point stride that keeps every record's time 8-aligned
    rec = dc.records(cloud[:, :3], 28, np.linspace(0, 0.1, len(cloud)), 16)
    d, k = _desc(ng, len(cloud), times=4, time_format=dm.TIME_F64_S)
    assert g._L.ngicp_deskew_cloud(g._h, rec.ctypes.data_as(c_f32p), len(rec), 28, C.byref(d), np.empty((len(rec), 3), np.float32).ctypes.data_as(c_f32p), 12) == ERR_ARG
    # the handle still works, through both entries
    (rc1, _), (rc2, _, m) = _call_both(g, cloud, valid)
    assert rc1 == 0 and rc2 == 0 and m > 0
    assert g._L.ngicp_set_source_preprocessed(g._h, 0) == 0
    del keep, keep_valid


def test_empty_cloud_is_a_no_op(ng):
    g = ng.NanoGICP()
    cloud = fc.scan_cloud(257, 34)
    d, keep = _desc(ng, 0, times=np.zeros(0, np.float32))
    g.preprocessScan(cloud, True, 1.0, 0.25, intensity_col=4)
    (rc1, _), (rc2, _, m) = _call_both(g, cloud[:0], d)
    assert rc1 == 0 and rc2 == 0 and m == 0
    assert g._L.ngicp_set_source_preprocessed(g._h, 0) == ERR_STATE  # as after ngicp_preprocess_scan with n = 0
    assert g.deskewCloud(cloud[:0], np.zeros(0), [0.0, 1.0], np.tile(np.eye(4), (2, 1, 1))).shape == (0, 3)
    del keep


def test_deskew_calls_leave_the_last_alignments_results_alone(ng):
    w = clouds.scan_to_scan(10_000)
    g = ng.NanoGICP()
    g.setMaxCorrespondenceDistance(1.0)
    g.setInputSource(w.source); g.setInputTarget(w.target)
    g.align()

    def getters():
        corr, sqd = g.correspondences()
        return [g.getSourceCovariances(), g.getTargetCovariances(), corr, sqd, np.asarray(g.lm_trace()), g.targetPoints(),
                g.transformSource(np.eye(4, dtype=np.float32)), np.float64(g.getFitnessScore()), np.float32(g.medianRange("source"))]
    before = getters()
    tau, poses = dc.random_trajectory(3, 35)
    s = clouds.sweep_times(len(w.source))
    g.deskewCloud(w.source, s, tau, poses, T_REF)
    g.preprocessScanDeskewed(w.source, s, tau, poses, T_REF, crop_size=1.0, voxel_res=0.25)
    with pytest.raises(ng.NgicpError):
        g.deskewCloud(w.source, s, tau[:1], poses[:1])
    for realign in (False, True):  # right after the deskew calls, and after the next align()
        if realign:
            g.align()
        for x, y in zip(before, getters()):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def test_deskew_cloud_leaves_a_pending_preprocessed_cloud_in_place(ng):
    a, b = ng.NanoGICP(), ng.NanoGICP()
    cloud = fc.scan_cloud(4097, 36)
    tau, poses = dc.random_trajectory(3, 37)
    for stages in ((True, 1.0, 0.25), (False, 0.0, 0.0)):  # a result in the filter workspace; a result that is the unpacked input itself
        for e in (a, b):
            e.preprocessScan(cloud, *stages, intensity_col=4)
        a.deskewCloud(points(6000, 38), np.linspace(0, 0.1, 6000), tau, poses)
        n_kept = len(fmodel.filter_cloud(cloud, *stages, 4))
        for rank in (0, n_kept // 2, n_kept - 1):
            assert a.rangeSelect(rank, "preprocessed").tobytes() == b.rangeSelect(rank, "preprocessed").tobytes()
        if stages[0]:  # (a cloud with non-finite rows cannot become the source)
            assert a._L.ngicp_set_source_preprocessed(a._h, 0) == 0


# ------------------------------------------------------------------ 5. end to end
def test_skewed_sweep_is_restored_and_aligns_like_the_undistorted_scan(ng):
    """A 3008-point scan distorted by a constant twist of 5 m/s and 1 rad/s over the 0.1 s sweep, deskewed with the true trajectory
    into the frame at the sweep's end, is the undistorted scan to 2 float32 ulps of the largest coordinate (the bound
    test_deskew_model_cpu.py derives: one rounding in each direction).  The alignments are reported, not asserted: measured 0.377 mm / 0.0014 deg from
    ground truth for the undistorted and for the deskewed scan, 93.7 mm / 2.06 deg for the raw skewed sweep."""
    w = clouds.scan_to_submap(3008)
    tau, poses = dc.twist_trajectory((5.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.1, 11)
    T_ref = poses[-1]
    s = clouds.sweep_times(len(w.source), sweep_s=0.1)
    raw = clouds.skew_scan(w.source, s, tau, poses, T_ref)
    g = ng.NanoGICP()
    back = g.deskewCloud(raw, s.astype(np.float32), tau, poses, T_ref)
    back64 = g.deskewCloud(raw, s, tau, poses, T_ref)
    bound = 2 * np.spacing(np.float32(max(np.abs(w.source).max(), np.abs(raw).max())))
    err64 = np.abs(back64.astype(np.float64) - w.source).max()
    print(f"distortion max {np.abs(raw - w.source).max():.3f} m; restored to {err64:.3e} m (bound {bound:.3e}); with float32 times {np.abs(back - w.source).max():.3e} m")
    assert err64 <= bound
    g.setMaxCorrespondenceDistance(w.max_corr_dist)
    g.setInputTarget(w.target)
    for name, cloud in (("undistorted", w.source), ("skewed", raw), ("deskewed", back64)):
        g.setInputSource(cloud)
        g.align(w.guess)
        dt, dr = clouds.pose_error(g.getFinalTransformation(), w.gt)
        print(f"align {name}: {dt * 1e3:.3f} mm, {np.degrees(dr):.4f} deg from ground truth, {g.nr_iterations_} iterations")
