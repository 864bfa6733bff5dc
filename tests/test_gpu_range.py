"""The exact device-side range select (-m gpu): ngicp_range_select / ngicp_range_median (include/ngicp.h "range select",
csrc/ngicp_range.h) through the Python API, against the numpy model of tests/_range_model.py, bit for bit
(`.view(np.uint32)`; a NaN answer matches any NaN: the engine returns the quiet NaN 0x7fc00000)."""
import numpy as np
import pytest

import _range_model as rm
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

DLO_CROP, DLO_LEAF = 1.0, 0.25  # cfg/params.yaml:28-33 of the reference


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _check(g, cloud, ranks, which="source"):
    d = np.sort(rm.ranges(cloud))  # NaN last
    for r in ranks:
        got = g.rangeSelect(r, which)
        assert isinstance(got, np.float32)
        assert rm.same_bits(got, d[r]), (len(cloud), r, got, d[r])
    assert rm.same_bits(g.medianRange(which), d[len(cloud) // 2])


def _xyzi(c):
    return np.ascontiguousarray(np.c_[c, np.zeros(len(c), np.float32)], np.float32)


# ------------------------------------------------------------------ wave, block and tile edges
@pytest.mark.parametrize("n", rm.EDGE_SIZES)
def test_sizes_around_wave_block_and_tile_edges(ng, n):
    c = rm.random_cloud(n)
    g = ng.NanoGICP()
    g.setInputSource(c)
    _check(g, c, rm.ranks_for(n))
    g.close()


# ------------------------------------------------------------------ where a round can go wrong
@pytest.mark.parametrize("case", ["all_equal", "low_bits_only", "top_bits_only"])
def test_digits_that_live_in_one_round_only(ng, case):
    c = getattr(rm, case)()
    g = ng.NanoGICP()
    g.setInputTarget(c)
    _check(g, c, rm.ranks_for(len(c)), "target")
    g.close()


def test_two_values_rank_on_either_side_of_the_boundary(ng):
    c = rm.two_values(301, 212)
    g = ng.NanoGICP()
    g.setInputSource(c)
    assert g.rangeSelect(300) == np.float32(5) and g.rangeSelect(301) == np.float32(13)
    _check(g, c, [0, 1, 299, 300, 301, 302, 511, 512])
    g.close()


def test_a_bin_with_more_than_65535_points(ng):
    c = rm.big_bin()
    g = ng.NanoGICP()
    g.setInputSource(c)
    _check(g, c, rm.ranks_for(len(c)))
    g.close()


# ------------------------------------------------------------------ rounding
def test_rounding_ties_of_the_root(ng):
    """4 096 points whose double sum is within one double ulp of a float rounding tie of the root, with the zero point, a denormal
    coordinate and 3e38: every rank, so every point's range is pinned.  The extremes go through the preprocessed scan (no index is
    built over 3e38); the ties alone also through an indexed source."""
    c = rm.rounding_ties()
    g = ng.NanoGICP()
    kept = g.preprocessScan(_xyzi(c), remove_nan=False, intensity_col=3)
    assert np.array_equal(kept[:, :3].view(np.uint32), c.view(np.uint32))
    d = np.sort(rm.ranges(c))
    got = np.array([g.rangeSelect(r, "preprocessed") for r in range(len(c))], np.float32)
    assert np.array_equal(got.view(np.uint32), d.view(np.uint32))
    ties = rm.rounding_ties(extremes=False)[:1500]
    g.setInputSource(ties)
    d = np.sort(rm.ranges(ties))
    got = np.array([g.rangeSelect(r) for r in range(0, len(ties), 3)], np.float32)
    assert np.array_equal(got.view(np.uint32), d[::3].view(np.uint32))
    g.close()


# ------------------------------------------------------------------ padding
@pytest.mark.parametrize("n", [3, 65])
def test_sentinel_rows_of_the_sorted_array_are_not_counted(ng, n):
    """The indexed clouds sit between two runs of far-away sentinel rows (csrc/ngicp_grid.h kSortedPad): the smallest and the largest
    range must be real points'."""
    c = rm.random_cloud(n, seed=3)
    d = rm.ranges(c)
    for which, setter in (("source", "setInputSource"), ("target", "setInputTarget")):
        g = ng.NanoGICP()
        getattr(g, setter)(c)
        assert rm.same_bits(g.rangeSelect(0, which), d.min()) and rm.same_bits(g.rangeSelect(n - 1, which), d.max())
        with pytest.raises(ng.NgicpError):
            g.rangeSelect(n, which)
        g.close()


# ------------------------------------------------------------------ the three clouds
def test_source_target_swap_and_registered_source(ng):
    w = clouds.scan_to_scan(10_000)
    g = ng.NanoGICP()
    g.setInputSource(w.source); g.setInputTarget(w.target)
    ranks_s, ranks_t = rm.ranks_for(len(w.source)), rm.ranks_for(len(w.target))
    _check(g, w.source, ranks_s, "source")
    _check(g, w.target, ranks_t, "target")
    g.swapSourceAndTarget()
    _check(g, w.target, ranks_t, "source")
    _check(g, w.source, ranks_s, "target")
    other = rm.random_cloud(1025, seed=8)
    g.registerInputSource(other)  # deferred upload: the entry uploads it first
    _check(g, other, rm.ranks_for(len(other)), "source")
    g.close()


def test_target_assembled_from_two_keyframes(ng):
    a, b = rm.random_cloud(2049, seed=1), rm.random_cloud(1023, seed=2)
    s2s, s2m = ng.NanoGICP(), ng.NanoGICP()
    for c in (a, b):
        s2s.setInputSource(c)
        s2s.calculateSourceCovariances()
        s2m.addKeyframe(s2s)
    assert s2m.setSubmapKeyframes([0, 1])
    both = np.concatenate([a, b])
    assert np.array_equal(s2m.targetPoints(), both)
    _check(s2m, both, rm.ranks_for(len(both)), "target")
    s2s.close(); s2m.close()


def test_preprocessed_scan_with_the_dlo_settings(ng):
    w = clouds.scan_to_scan(10_000)
    g = ng.NanoGICP()
    filtered = g.preprocessScan(clouds.to_xyzi(w.source), True, DLO_CROP, DLO_LEAF, intensity_col=4)
    assert 0 < len(filtered) < len(w.source)
    _check(g, filtered[:, :3], rm.ranks_for(len(filtered)), "preprocessed")
    before = g.medianRange("preprocessed")
    # ... and once it is the source (setInputSourcePreprocessed: the scan never left the device) the source gives the same value
    g.preprocessScan(clouds.to_xyzi(w.source), True, DLO_CROP, DLO_LEAF, intensity_col=4, set_as_source=True)
    assert rm.same_bits(g.medianRange("source"), before)
    _check(g, filtered[:, :3], rm.ranks_for(len(filtered)), "source")
    g.close()


def test_preprocessed_scan_keeps_nonfinite_rows_nan_last(ng):
    c, n_nan, n_inf = rm.with_nonfinite_rows()
    g = ng.NanoGICP()
    kept = g.preprocessScan(_xyzi(c), remove_nan=False, intensity_col=3)
    assert len(kept) == len(c)
    n = len(c)
    _check(g, c, [0, n // 2, n - n_nan - n_inf - 1, *range(n - n_nan - n_inf, n)], "preprocessed")
    assert np.isnan(g.rangeSelect(n - 1, "preprocessed")) and np.isnan(g.rangeSelect(n - n_nan, "preprocessed"))
    assert g.rangeSelect(n - n_nan - 1, "preprocessed") == np.inf and g.rangeSelect(n - n_nan - n_inf, "preprocessed") == np.inf
    assert np.isfinite(g.rangeSelect(n - n_nan - n_inf - 1, "preprocessed"))
    g.close()


# ------------------------------------------------------------------ nothing else moves
def _pair(ng, w):
    g = ng.NanoGICP()
    g.setMaxCorrespondenceDistance(1.0)
    g.setInputSource(w.source); g.setInputTarget(w.target)
    return g


def test_linearize_results_survive_a_range_select(ng):
    w = clouds.scan_to_scan(10_000)
    g = _pair(ng, w)
    T = np.eye(4)
    H, b, e = g.linearize(T)
    corr, sqd = g.correspondences()
    err = g.compute_error(T)
    for which in ("source", "target"):
        g.rangeSelect(17, which); g.medianRange(which)
    corr2, sqd2 = g.correspondences()
    assert np.array_equal(corr, corr2) and np.array_equal(sqd, sqd2)
    assert g.compute_error(T) == err
    H2, b2, e2 = g.linearize(T)
    assert np.array_equal(H, H2) and np.array_equal(b, b2) and e == e2
    g.close()


def test_pending_radius_search_survives_a_range_select(ng):
    w = clouds.scan_to_scan(10_000)
    g, ref = _pair(ng, w), _pair(ng, w)
    q = np.ascontiguousarray(w.source[::503])
    off_ref, idx_ref, d2_ref = ref.radiusSearch(q, 0.09)
    assert idx_ref.size > 0
    # the search's results wait on the device for ngicp_radius_fetch: a range select in between must leave them alone
    L, C = g._L, ng.C
    offsets = np.zeros(len(q) + 1, np.uint64)
    total = C.c_size_t(0)
    g._ck(L.ngicp_radius_search(g._h, 1, q.ctypes.data_as(ng.c_f32p), len(q), q.strides[0], 0.09, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(total)))
    g.medianRange("source"); g.rangeSelect(0, "target")
    idx = np.empty(total.value, np.int32); d2 = np.empty(total.value, np.float32)
    g._ck(L.ngicp_radius_fetch(g._h, idx.ctypes.data_as(ng.c_i32p), d2.ctypes.data_as(ng.c_f32p), total.value))
    assert np.array_equal(offsets.astype(np.int64), off_ref) and np.array_equal(idx, idx_ref) and np.array_equal(d2, d2_ref)
    g.close(); ref.close()


def test_align_is_the_same_with_range_selects_around_it(ng):
    w = clouds.scan_to_scan(10_000)
    g, ref = _pair(ng, w), _pair(ng, w)
    ref.align()
    m0 = g.medianRange("source")
    g.align()
    m1 = g.medianRange("source")
    assert rm.same_bits(m0, m1) and rm.same_bits(m0, rm.median(w.source))
    assert np.array_equal(g.getFinalTransformation(), ref.getFinalTransformation())
    assert g.nr_iterations_ == ref.nr_iterations_ and g.converged_ == ref.converged_
    assert np.array_equal(g.getFinalHessian(), ref.getFinalHessian())
    c_g, c_ref = g.correspondences()[0], ref.correspondences()[0]
    assert np.array_equal(c_g, c_ref)
    assert g.getFitnessScore() == ref.getFitnessScore()
    g.align()  # and again after the select
    assert np.array_equal(g.getFinalTransformation(), ref.getFinalTransformation())
    g.close(); ref.close()


def test_preprocessed_scan_is_still_usable_after_a_range_select(ng):
    w = clouds.scan_to_scan(10_000)
    a, b = ng.NanoGICP(), ng.NanoGICP()
    cloud = clouds.to_xyzi(w.source)
    for g in (a, b):
        g.preprocessScan(cloud, True, DLO_CROP, DLO_LEAF, intensity_col=4)
    a.medianRange("preprocessed")
    for g in (a, b):
        g._ck(g._L.ngicp_set_source_preprocessed(g._h, 0))
        g.calculateSourceCovariances()
    assert np.array_equal(a.getSourceCovariances(), b.getSourceCovariances())
    a.close(); b.close()


# ------------------------------------------------------------------ errors
def test_errors_and_the_handle_stays_usable(ng):
    g = ng.NanoGICP()
    for which in ("source", "target", "preprocessed"):
        with pytest.raises(ng.NgicpError) as e:
            g.rangeSelect(0, which)
        assert e.value.code == -3  # NGICP_ERR_STATE: nothing there
        with pytest.raises(ng.NgicpError) as e:
            g.medianRange(which)
        assert e.value.code == -3
    c = rm.random_cloud(257)
    g.setInputSource(c)
    for bad_rank in (257, 258, 2 ** 40):
        with pytest.raises(ng.NgicpError) as e:
            g.rangeSelect(bad_rank)
        assert e.value.code == -2  # NGICP_ERR_ARG
    with pytest.raises(ng.NgicpError) as e:
        g.rangeSelect(0, "keyframes")
    assert e.value.code == -2
    v, n = ng.C.c_float(0), ng.C.c_size_t(0)
    for which in (-1, 3):
        assert g._L.ngicp_range_select(g._h, which, 0, ng.C.byref(v), None) == -2
        assert g._L.ngicp_range_median(g._h, which, ng.C.byref(v), None) == -2
    assert g._L.ngicp_range_select(g._h, 0, 0, None, None) == -2  # null value
    assert g._L.ngicp_range_select(g._h, 0, 256, ng.C.byref(v), ng.C.byref(n)) == 0 and n.value == 257
    assert rm.same_bits(v.value, rm.select(c, 256))
    # the preprocessed scan is gone once a later call has consumed the filter workspace, exactly when setInputSourcePreprocessed refuses
    w = clouds.scan_to_scan(10_000)
    s2m = ng.NanoGICP()
    g.preprocessScan(clouds.to_xyzi(w.source), True, DLO_CROP, DLO_LEAF, intensity_col=4, set_as_source=True)
    g.medianRange("preprocessed")
    s2m.addKeyframeTransformedFiltered(g, np.eye(4), 0.5)
    with pytest.raises(ng.NgicpError) as e:
        g.medianRange("preprocessed")
    assert e.value.code == -3
    assert g._L.ngicp_set_source_preprocessed(g._h, 0) == -3
    # ... and the handle works on
    filtered = g.preprocessScan(clouds.to_xyzi(w.source), True, DLO_CROP, DLO_LEAF, intensity_col=4, set_as_source=True)
    assert rm.same_bits(g.medianRange("preprocessed"), rm.median(filtered[:, :3]))
    assert rm.same_bits(g.medianRange("source"), rm.median(filtered[:, :3]))
    g.setInputTarget(w.target)
    g.align()
    assert g.converged_
    g.close(); s2m.close()


# ------------------------------------------------------------------ one workload-sized case
def test_median_of_a_250k_point_scan(ng):
    scan = clouds.os1_128(clouds.make_scene(), clouds.make_pose(), noise_seed=1, n=250_000)
    scan = np.ascontiguousarray(scan[:, :3], np.float32)
    assert len(scan) >= 200_000
    g = ng.NanoGICP()
    g.setInputSource(scan)
    assert rm.same_bits(g.medianRange(), rm.median(scan))
    _check(g, scan, [0, len(scan) - 1])
    assert g.stats()["query_ms"] > 0
    g.close()
