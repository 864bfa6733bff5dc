"""GPU tests (-m gpu) of the filter pipeline (csrc/ngicp_filters.hip: flags, three-kernel scan, order-preserving compaction, lattice,
stable LSD radix sort with a pass count carried between calls, segment heads, serial centroids) and of the ABI around it
(ngicp_preprocess_scan, ngicp_set_source_preprocessed, ngicp_map_*, ngicp_keyframe_add_transformed_filtered).

Checkers: the oracle's C++ restatement AND the independent numpy model (tests/_filter_model.py), which test_filter_cases_cpu.py proves
against each other on every case of tests/_filter_cases.py.  Every comparison is bit for bit (NaN equal to NaN where a NaN intensity
is the expected centroid); no tolerance is involved.  Every case is valid input or a refused argument."""
import ctypes as C

import numpy as np
import pytest

import _filter_cases as fc
import _filter_model as model
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_K_TOO_LARGE = -2, -3, -4  # include/ngicp.h
c_f32p = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _run(g, c):
    return g.preprocessScan(c.cloud, remove_nan=c.remove_nan, crop_size=c.crop, voxel_res=c.leaf, intensity_col=c.icol)


def _case(cloud, remove_nan, crop, leaf, icol=4, name="adhoc"):
    return fc.Case(name, np.ascontiguousarray(cloud, dtype=np.float32), icol, remove_nan, crop, leaf)


def _check(g, c, what=""):
    got = _run(g, c)
    exp = model.filter_cloud(c.cloud, c.remove_nan, c.crop, c.leaf, c.icol)
    assert got.shape == exp.shape, f"{what}: {got.shape} vs the model's {exp.shape}"
    assert fc.same(c, got, exp), what
    return got


# ------------------------------------------------------------------ every case, fresh handle
@pytest.mark.parametrize("name", fc.names())
def test_case_matches_oracle_and_model(ng, oracle_mod, name):
    c = fc.by_name(name)
    got = _run(ng.NanoGICP(), c)
    ref = oracle_mod.filter_cloud(c.cloud, c.remove_nan, c.crop, c.leaf, intensity_col=c.icol)
    exp = fc.expected(name)
    print(f"{name}: {len(c.cloud)} rows -> engine {len(got)}, oracle {len(ref)}, model {len(exp)}")
    assert got.shape == ref.shape == exp.shape
    assert fc.same(c, got, exp)
    assert fc.same(c, got, ref)


# ------------------------------------------------------------------ call sequences on one handle (FilterWorkspace::last_bits)
# class of the call (E of fc.keybits_cloud): 8 = <= 11 key bits, 100 = 12-22, 1000 = 23-31, 1291 = overflow.  Transitions, in order:
#   8 -> 100 re-run | 100 -> 1000 re-run again | 1000 -> 8 class switch only | 8 -> 100 re-run | 100 -> 8 copy passes |
#   8 -> 1291 overflow (last_bits must survive) | 1291 -> 100 the pass count of the call before the overflow is reused (re-run)
SEQUENCE = (8, 100, 1000, 8, 100, 8, 1291, 100)


@pytest.mark.parametrize("sizes", [(5002,) * 8, (8193, 65, 4097, 1, 600_001, 1025, 8193, 65)], ids=["same-size", "shrinking-growing"])
def test_keybit_class_sequence_on_one_handle(ng, sizes):
    """The sort enqueues the passes the PREVIOUS call needed and runs again when that was too few; passes above the highest bit in use
    copy.  Sizes that shrink and grow between the calls reuse the buffers of a larger call and reallocate them mid-sequence."""
    g = ng.NanoGICP()
    for step, (E, n) in enumerate(zip(SEQUENCE, sizes)):
        c = _case(fc.keybits_cloud(E, n, 900 + step), True, 0.0, 1.0)
        got = _check(g, c, f"step {step}: E = {E}, n = {n}")
        if E == 1291 and n >= 3:
            assert len(got) == n  # returned as it is


def test_copy_passes_after_a_wider_call_and_back(ng):
    """23-31 bits, then <= 11 (two copy passes), then 12-22 (one copy pass), then 23-31 again, each twice (steady state in between)."""
    g = ng.NanoGICP()
    for step, E in enumerate((1000, 8, 8, 100, 100, 1000, 1000, 8)):
        _check(g, _case(fc.keybits_cloud(E, 3000 + 517 * step, 950 + step), True, 0.0, 1.0), f"step {step}: E = {E}")


# ------------------------------------------------------------------ the three users of one workspace, as DLO interleaves them per frame
def _pair(ng, k=10):
    s2s, s2m = ng.NanoGICP(), ng.NanoGICP()
    s2s.setCorrespondenceRandomness(k)
    return s2s, s2m


def test_scan_keyframe_and_map_filters_interleaved_on_one_workspace(ng, oracle_mod):
    """Per frame: preprocessScan (crop 1.0, leaf 0.25) -> the filtered scan becomes the source -> addKeyframeTransformedFiltered (leaf
    0.5) from that producer -> mapAdd -> mapVoxelFilter (leaf 0.3) on the producer's handle: all three filter through the producer's
    workspace and its last_bits.  Three frames of different sizes; every result against the model."""
    s2s, s2m = _pair(ng)
    host_map = np.zeros((0, 4), np.float32)
    for frame, n in enumerate((9001, 2500, 20_011)):
        scan = fc.scan_cloud(n, 300 + frame)
        c = _case(scan, True, 1.0, 0.25)
        exp = model.filter_cloud(scan, True, 1.0, 0.25, 4)
        got = s2s.preprocessScan(scan, True, 1.0, 0.25, intensity_col=4, set_as_source=True)
        assert fc.same(c, got, exp), f"frame {frame}: scan"
        T = clouds.make_pose((0.4 + frame, -0.2, 0.05), (0.5, -0.3, 3.0 * frame)).astype(np.float32)
        kid = s2m.addKeyframeTransformedFiltered(s2s, T, 0.5)
        moved = oracle_mod.transform_cloud(np.ascontiguousarray(exp[:, :3]), T)
        kf = model.filter_cloud(np.c_[moved, np.zeros(len(moved), np.float32)], False, 0.0, 0.5, 3)
        assert s2m.keyframeSize(kid) == len(kf) and s2m.numKeyframes() == frame + 1
        s2m.setSubmapKeyframes([kid])
        assert fc.same_bits(s2m.targetPoints(), kf[:, :3]), f"frame {frame}: keyframe"
        s2s.mapAdd(got, intensity_col=3)
        host_map = model.filter_cloud(np.concatenate([host_map, got]), False, 0.0, 0.3, 3)
        assert s2s.mapVoxelFilter(0.3) == len(host_map)
        assert fc.same_bits(s2s.mapGet(), host_map), f"frame {frame}: map"


def test_keyframe_filter_between_preprocess_and_set_source_is_refused(ng):
    """addKeyframeTransformedFiltered filters through the PRODUCER's workspace: a preprocessed scan waiting there is gone, and the
    hand-over must be refused rather than index reused memory (the map variant: test_gpu_submap.py)."""
    s2s, s2m = _pair(ng)
    scan = fc.scan_cloud(6000, 310)
    s2s.preprocessScan(scan, True, 1.0, 0.25, intensity_col=4, set_as_source=True)
    s2s.preprocessScan(fc.scan_cloud(5000, 311), True, 1.0, 0.25, intensity_col=4)  # waits in the workspace
    s2m.addKeyframeTransformedFiltered(s2s, np.eye(4, dtype=np.float32), 0.5)
    assert s2s._L.ngicp_set_source_preprocessed(s2s._h, 0) == ERR_STATE
    _check(s2s, _case(scan, True, 1.0, 0.25), "the ordinary order afterwards")
    assert s2s._L.ngicp_set_source_preprocessed(s2s._h, 0) == 0


# ------------------------------------------------------------------ ABI shapes, through the C entry points themselves
def _raw(g, buf, n, stride, ioff, remove_nan, crop, leaf, out, cap):
    m = C.c_size_t(12345)
    rc = g._L.ngicp_preprocess_scan(g._h, buf.ctypes.data_as(c_f32p) if buf is not None else None, n, stride, ioff, 1 if remove_nan else 0, crop, leaf,
                                    out.ctypes.data_as(c_f32p) if out is not None else None, cap, C.byref(m))
    return rc, m.value


def _layout(cloud32, stride, ioff):
    """The 32-byte cloud re-laid with `stride` bytes per row, the intensity at byte `ioff` (none for -1), the padding filled with junk."""
    n = len(cloud32)
    buf = np.full((n, stride // 4), 777.0, np.float32)
    buf[:, :3] = cloud32[:, :3]
    if ioff >= 0:
        buf[:, ioff // 4] = cloud32[:, 4]
    return buf


@pytest.mark.parametrize("stages", [(True, 1.0, 0.25), (False, 0.0, 0.0)], ids=["crop-leaf", "raw"])
def test_stride_and_offset_layouts_give_the_same_output(ng, stages):
    rn, crop, leaf = stages
    cloud = fc.scan_cloud(1025, 400)
    exp = model.filter_cloud(cloud, rn, crop, leaf, 4)
    c = _case(cloud, rn, crop, leaf)
    g = ng.NanoGICP()
    for stride, ioff in ((12, -1), (16, 12), (32, 16), (48, 44), (12, -1), (48, 12)):
        buf = _layout(cloud, stride, ioff)
        out = np.full((len(cloud), 4), -5.0, np.float32)
        rc, m = _raw(g, buf, len(cloud), stride, ioff, rn, crop, leaf, out, len(out))
        assert rc == 0 and m == len(exp), (stride, ioff)
        want = exp if ioff >= 0 else model.filter_cloud(cloud, rn, crop, leaf, None)
        assert fc.same(c, out[:m], want), (stride, ioff)
        if ioff < 0:
            assert fc.same_bits(out[:m, :3], exp[:, :3], nan_equal=True) and (out[:m, 3].view(np.uint32) == 0).all()
        assert (out[m:] == -5.0).all()


def test_bad_strides_and_offsets_are_refused(ng):
    cloud = fc.scan_cloud(257, 401)
    buf = _layout(cloud, 48, 44)  # large enough for every layout tried below
    out = np.empty((len(cloud), 4), np.float32)
    g = ng.NanoGICP()
    for stride, ioff in ((10, -1), (14, -1), (16, 16), (32, 32), (32, 6), (8, -1), (12, 12)):
        rc, m = _raw(g, buf, len(cloud), stride, ioff, True, 1.0, 0.25, out, len(out))
        assert rc == ERR_ARG and m == 0, (stride, ioff)
        assert g._L.ngicp_set_source_preprocessed(g._h, 0) == ERR_STATE
        rc, m = g._L.ngicp_map_add(g._h, buf.ctypes.data_as(c_f32p), len(cloud), stride, ioff), g.mapSize()
        assert rc == ERR_ARG and m == 0, (stride, ioff)
    _check(g, _case(cloud, True, 1.0, 0.25), "after the refused calls")


def test_output_buffer_null_short_and_empty_input(ng):
    cloud = fc.scan_cloud(4097, 402)
    exp = model.filter_cloud(cloud, True, 1.0, 0.25, 4)
    c = _case(cloud, True, 1.0, 0.25)
    g = ng.NanoGICP()
    # no output buffer: the count alone, and the filtered cloud can still become the source
    rc, m = _raw(g, cloud, len(cloud), 32, 16, True, 1.0, 0.25, None, 0)
    assert rc == 0 and m == len(exp)
    assert g._L.ngicp_set_source_preprocessed(g._h, 0) == 0
    g._src = np.ascontiguousarray(exp[:, :3])
    assert fc.same_bits(g.transformSource(np.eye(4, dtype=np.float32)), exp[:, :3])  # x * 1 + (y * 0 + (z * 0 + 0)): the source, in its order
    # a capacity one short is refused, nothing is written, and the next call works
    out = np.full((len(exp), 4), -5.0, np.float32)
    rc, m = _raw(g, cloud, len(cloud), 32, 16, True, 1.0, 0.25, out, len(exp) - 1)
    assert rc == ERR_ARG and (out == -5.0).all()
    rc, m = _raw(g, cloud, len(cloud), 32, 16, True, 1.0, 0.25, out, len(exp))
    assert rc == 0 and m == len(exp) and fc.same(c, out, exp)
    # n = 0, with and without pointers
    for buf in (cloud, None):
        rc, m = _raw(g, buf, 0, 32, 16, True, 1.0, 0.25, out, len(out))
        assert rc == 0 and m == 0
        assert g._L.ngicp_set_source_preprocessed(g._h, 0) == ERR_STATE
    _check(g, c, "after the empty calls")


@pytest.mark.parametrize("name", [n for n in fc.names() if n.startswith("nothing-survives")])
def test_nothing_survives_then_the_handle_stays_usable(ng, name):
    c = fc.by_name(name)
    g = ng.NanoGICP()
    out = np.full((len(c.cloud), 4), -5.0, np.float32)
    rc, m = _raw(g, c.cloud, len(c.cloud), 32, 16, c.remove_nan, c.crop, c.leaf, out, len(out))
    assert rc == 0 and m == 0 and (out == -5.0).all()
    assert g._L.ngicp_set_source_preprocessed(g._h, 0) == ERR_STATE
    usable = fc.by_name("n1025-nan_crop_leaf")
    got = g.preprocessScan(usable.cloud, True, 1.0, 0.25, intensity_col=4, set_as_source=True)
    assert fc.same(usable, got, fc.expected(usable.name))


# ------------------------------------------------------------------ map
def test_map_grows_in_odd_pieces_and_filters_as_the_model_says(ng):
    rng = np.random.default_rng(500)
    g = ng.NanoGICP()
    host = np.zeros((0, 4), np.float32)
    for n in (1, 63, 1025, 4097, 1):  # crosses the doubling growth and its device-to-device copy several times
        piece = np.c_[(rng.uniform(-1, 1, (n, 3)) * 15.0), rng.uniform(0, 255, n)].astype(np.float32)
        g.mapAdd(piece, intensity_col=3)
        host = np.concatenate([host, piece])
        assert g.mapSize() == len(host)
        assert fc.same_bits(g.mapGet(), host)
    for leaf in (0.0, -1.0):  # no-op
        assert g.mapVoxelFilter(leaf) == len(host) and fc.same_bits(g.mapGet(), host)
    host = model.filter_cloud(host, False, 0.0, 0.3, 3)
    assert g.mapVoxelFilter(0.3) == len(host) and len(host) < 5187
    assert fc.same_bits(g.mapGet(), host)
    piece = np.c_[(rng.uniform(-1, 1, (3000, 3)) * 15.0), rng.uniform(0, 255, 3000)].astype(np.float32)  # add after a filter, filter again
    g.mapAdd(piece, intensity_col=3)
    host = np.concatenate([host, piece])
    assert fc.same_bits(g.mapGet(), host)
    host = model.filter_cloud(host, False, 0.0, 0.5, 3)
    assert g.mapVoxelFilter(0.5) == len(host)
    assert fc.same_bits(g.mapGet(), host)
    g.mapClear()
    assert g.mapSize() == 0 and g.mapVoxelFilter(0.3) == 0


def test_map_with_nan_rows(ng):
    """VoxelGrid skips the non-finite rows; on overflow it returns its input, and the map - NaN rows included - stays as it is."""
    u = fc.by_name("unusual-raw")
    rows = model.unpack(u.cloud, 4)
    g = ng.NanoGICP()
    g.mapAdd(rows, intensity_col=3)
    assert fc.same_bits(g.mapGet(), rows)
    for leaf in (1e-9, 1e-12):
        assert g.mapVoxelFilter(leaf) == len(rows)
        assert fc.same_bits(g.mapGet(), rows)
    exp = model.filter_cloud(rows, False, 0.0, 0.5, 3)
    assert g.mapVoxelFilter(0.5) == len(exp) < len(rows)
    assert fc.same_bits(g.mapGet(), exp, nan_equal=True)


# ------------------------------------------------------------------ keyframe route at small sizes
def test_filtered_keyframe_smaller_than_k_is_refused_and_changes_nothing(ng):
    w = clouds.scan_to_scan(10_000)
    src = np.ascontiguousarray(w.source[:300])
    s2s, s2m = _pair(ng, k=20)
    for e in (s2s, s2m):
        e.setMaxCorrespondenceDistance(1.0)
    s2s.setInputSource(src)
    T = np.eye(4, dtype=np.float32)
    kid = s2m.addKeyframeTransformedFiltered(s2s, T, 0.5)
    before = s2m.numKeyframes()
    leaf = 1e4  # a handful of voxels at most: fewer points than the producer's k = 20
    left = len(model.filter_cloud(np.c_[src, np.zeros(300, np.float32)], False, 0.0, leaf, 3))
    assert 0 < left < 20
    with pytest.raises(ng.NgicpError) as ei:
        s2m.addKeyframeTransformedFiltered(s2s, T, leaf)
    assert ei.value.code == ERR_K_TOO_LARGE
    assert s2m.numKeyframes() == before == kid + 1
    # both handles still align: the producer against its own scan, the consumer against the keyframe it already holds
    s2s.setInputTarget(src)
    s2s.align()
    ref = ng.NanoGICP(); ref.setCorrespondenceRandomness(20); ref.setMaxCorrespondenceDistance(1.0)
    ref.setInputSource(src); ref.setInputTarget(src); ref.align()
    assert np.array_equal(s2s.getFinalTransformation(), ref.getFinalTransformation())
    s2m.setCorrespondenceRandomness(10)
    s2m.setInputSource(src)
    s2m.setSubmapKeyframes([kid])
    s2m.align()
    assert np.isfinite(s2m.getFinalTransformation()).all()
    assert s2m.addKeyframeTransformedFiltered(s2s, T, 0.5) == kid + 1
