"""The query surface beyond the registration path (-m gpu): getFitnessScore, k-NN on either index and radius search
(include/ngicp.h "queries", csrc/ngicp_query.h), against numpy brute force and the oracle's kd-tree.  Per-point squared
distances are float32 (dx*dx + dy*dy) + dz*dz without FMA, compared bit for bit; radius results come in ascending
(d2, original index) order."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

DBL_MAX = sys.float_info.max
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture(scope="module")
def ref_kdtree():
    with np.load(os.path.join(GOLDEN, "ref_kdtree.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _d2_rows(pts, q):
    """float32 squared distances of every query row to every point, in the engine's association (no FMA in numpy)."""
    dx = q[:, 0:1] - pts[None, :, 0]
    dy = q[:, 1:2] - pts[None, :, 1]
    dz = q[:, 2:3] - pts[None, :, 2]
    d = dx * dx
    d = d + dy * dy
    return d + dz * dz


def _nn_d2(pts, q, chunk=256):
    pts = np.ascontiguousarray(pts[:, :3], np.float32)
    q = np.ascontiguousarray(q[:, :3], np.float32)
    out = np.empty(len(q), np.float32)
    for s in range(0, len(q), chunk):
        out[s:s + chunk] = _d2_rows(pts, q[s:s + chunk]).min(axis=1)
    return out


def _fitness_ref(d2, max_range):
    d = d2.astype(np.float64)
    inl = d[d <= max_range]
    return (math.fsum(inl) / len(inl) if len(inl) else DBL_MAX), len(inl)


def _check_fitness(g, d2, max_range, T=None):
    """n_inliers exact; score within 1e-12 of the exactly rounded mean: the engine sums positive doubles in a fixed order (per lane,
    per wave, per block, then over a few thousand block partials), whose error is within about 1e-13 relative of the exact sum."""
    score, n = g.fitness(max_range, T)
    ref, nref = _fitness_ref(d2, max_range)
    assert n == nref
    if nref == 0:
        assert score == DBL_MAX
    else:
        assert abs(score - ref) <= 1e-12 * ref
    assert g.fitness(max_range, T) == (score, n)  # bit-identical from call to call
    return score, n


def _transformed(g, oracle_mod, src, T):
    tr = oracle_mod.transform_cloud(src, T)
    assert np.array_equal(tr, g.transformSource(T))  # the engine's transform is transform_point_f: bit-equal
    return tr


# ------------------------------------------------------------------ fitness
def test_fitness_vs_bruteforce_small(ng, oracle_mod, golden):
    w = clouds.scan_to_scan(10_000)
    cases = [(golden["source"], golden["target"], golden["guess"], float(golden["max_corr_dist"])), (w.source, w.target, w.guess, 1.0)]
    for src, tgt, guess, corr in cases:
        g = ng.NanoGICP(); g.setMaxCorrespondenceDistance(corr)
        g.setInputSource(src); g.setInputTarget(tgt)
        g.align(guess)
        T = g.getFinalTransformation()
        d2 = _nn_d2(tgt, _transformed(g, oracle_mod, src, T))
        for max_range in (DBL_MAX, corr * corr, 0.01):
            score, n = _check_fitness(g, d2, max_range)
            assert 0 < n <= len(src)
            assert g.getFitnessScore(max_range) == score


@pytest.fixture(scope="module")
def c3(ng):
    """The bench's workload (bench.py: scan_to_submap 100k -> 500k, k = 20, 20 iterations) and a handle aligned on it."""
    w = clouds.scan_to_submap(100_000, 5)
    tgt_covs = ng.keyframe_covariances(w.target, w.keyframe_sizes, 20)

    def make():
        g = ng.NanoGICP()
        g.setCorrespondenceRandomness(20); g.setMaxCorrespondenceDistance(w.max_corr_dist)
        g.setMaximumIterations(20); g.setTransformationEpsilon(1e-12); g.setRotationEpsilon(1e-12)
        g.setInputTarget(w.target); g.setTargetCovariances(tgt_covs)
        g.setInputSource(w.source); g.calculateSourceCovariances()
        g.align(w.guess)
        return g
    return w, make


def test_fitness_full_size(ng, oracle_mod, c3):
    w, make = c3
    g = make()
    T = g.getFinalTransformation()
    tr = _transformed(g, oracle_mod, w.source, T)
    d2 = oracle_mod.OracleTree(w.target).knn(tr, 1)[1][:, 0]  # the 1-NN distance does not depend on the tie order
    for max_range in (DBL_MAX, w.max_corr_dist ** 2):
        _check_fitness(g, d2, max_range)


def test_fitness_max_range_edges_and_state(ng, oracle_mod):
    w = clouds.scan_to_scan(10_000)
    src, tgt = w.source[:, :3].copy(), w.target[:, :3].copy()
    g = ng.NanoGICP(); g.setInputSource(src); g.setInputTarget(tgt)
    I = np.eye(4, dtype=np.float32)
    # before any align: final_transformation_ is the identity (PCL)
    d2_I = _nn_d2(tgt, src)
    assert g.fitness() == g.fitness(T=I)
    _check_fitness(g, d2_I, DBL_MAX)
    # max_range is compared with d2 in double, inclusive: one observed d2 counts at max_range == d2 and not just below it
    v = float(np.sort(d2_I)[len(d2_I) // 2])
    n_at = g.fitness(v)[1]
    n_below = g.fitness(float(np.nextafter(v, 0.0)))[1]
    assert n_at == int((d2_I.astype(np.float64) <= v).sum()) and n_below == int((d2_I.astype(np.float64) < v).sum()) and n_at > n_below
    # after an align, NULL is the final transform, and passing that transform explicitly is the same call
    g.align()
    T = g.getFinalTransformation()
    assert g.fitness() == g.fitness(T=T) and g.fitness(0.04) == g.fitness(0.04, T)
    _check_fitness(g, _nn_d2(tgt, _transformed(g, oracle_mod, src, T)), 0.04)
    # swapSourceAndTarget: the roles swap
    g.swapSourceAndTarget()
    _check_fitness(g, _nn_d2(src, _transformed(g, oracle_mod, tgt, T)), DBL_MAX, T)
    # disjoint clouds, max_range 0: nothing counts
    far = ng.NanoGICP(); far.setInputSource(src); far.setInputTarget(tgt + np.float32(100.0))
    assert far.fitness(0.0) == (DBL_MAX, 0)
    assert far.getFitnessScore(0.0) == DBL_MAX
    # a device-assembled submap target gives what the same points uploaded as a host cloud give
    prod = ng.NanoGICP()
    kf = [tgt[:4000], tgt[4000:]]
    sub = ng.NanoGICP()
    for c in kf:
        prod.setInputSource(np.ascontiguousarray(c)); sub.addKeyframe(prod)
    sub.setSubmapKeyframes([1, 0])
    sub.setInputSource(src)
    host = ng.NanoGICP(); host.setInputSource(src); host.setInputTarget(np.concatenate([kf[1], kf[0]]))
    for mr in (DBL_MAX, 0.04):
        assert sub.fitness(mr, T) == host.fitness(mr, T)
    # the source must be set
    empty = ng.NanoGICP(); empty.setInputTarget(tgt)
    with pytest.raises(ng.NgicpError) as e:
        empty.fitness()
    assert e.value.code == -3


# ------------------------------------------------------------------ k-NN on the source index
@pytest.mark.parametrize("key,k", [("n101_k20", 20), ("n5000_k1", 1), ("n5000_k20", 20), ("n20000_k32", 32)])
def test_knn_source_index_vs_reference(ng, ref_kdtree, key, k):
    """The reference kd-tree's stored answers (tests/golden/ref_kdtree.npz), the clouds set as the SOURCE: distances bit-exact, an
    index may differ only on an exact distance tie (SURVEY.md §7 "Ties"), as for the target index."""
    pts, q = ref_kdtree[key + "_pts"], ref_kdtree[key + "_q"]
    g = ng.NanoGICP(); g.setInputSource(pts)
    gi, gd = g.nearestKSearch(q, k, which="source")
    oi, od = ref_kdtree[key + "_idx"], ref_kdtree[key + "_d2"]
    assert np.array_equal(gd, od)
    same = gi == oi
    assert np.all(gd[~same] == od[~same]) and same.mean() > 0.999


def test_knn_source_index_ties_and_errors(ng, ref_kdtree):
    pts, q, oi, od = (ref_kdtree["ties_" + s] for s in ("pts", "q", "idx", "d2"))
    g = ng.NanoGICP(); g.setInputSource(pts)
    gi, gd = g.nearestKSearch(q, 8, which="source")
    assert np.array_equal(gd, od)
    for r in range(len(q)):  # ties: index SETS among the strictly-closer-than-kth neighbours
        assert set(gi[r][gd[r] < gd[r, -1]]) == set(oi[r][od[r] < od[r, -1]])
    # the target entry is the same search on the other slot
    g.setInputTarget(pts)
    ti, td = g.nearestKSearch(q, 8, which="target")
    assert np.array_equal(ti, gi) and np.array_equal(td, gd)
    assert all(np.array_equal(a, b) for a, b in zip(g.target_knn(q, 8), (ti, td)))
    small = ng.NanoGICP(); small.setInputSource(ref_kdtree["n7_k3_pts"])
    for kk in (33, 8):
        with pytest.raises(ng.NgicpError) as e:
            (g if kk == 33 else small).nearestKSearch(q, kk, which="source")
        assert e.value.code == -4
    qq = np.ascontiguousarray(q[:4], np.float32)
    idx = np.empty((4, 3), np.int32); d2 = np.empty((4, 3), np.float32)
    f32, i32 = C.POINTER(C.c_float), C.POINTER(C.c_int)
    assert g._L.ngicp_knn_search(g._h, 2, qq.ctypes.data_as(f32), 4, 12, 3, idx.ctypes.data_as(i32), d2.ctypes.data_as(f32)) == -2
    with pytest.raises(ng.NgicpError) as e:
        ng.NanoGICP().nearestKSearch(q, 3, which="source")
    assert e.value.code == -3


# ------------------------------------------------------------------ radius search
def _radius_ref(pts, q, radius):
    pts = np.ascontiguousarray(pts[:, :3], np.float32)
    r = np.float32(radius)
    offs, idx, d2 = [0], [], []
    for s in range(0, len(q), 64):
        d = _d2_rows(pts, np.ascontiguousarray(q[s:s + 64, :3], np.float32))
        for row in d:
            hit = np.nonzero(row < r)[0]
            o = np.lexsort((hit, row[hit]))  # ascending (d2, original index)
            idx.append(hit[o].astype(np.int32)); d2.append(row[hit][o])
            offs.append(offs[-1] + len(hit))
    cat = (lambda a, t: np.concatenate(a).astype(t) if a else np.empty(0, t))
    return np.array(offs, np.int64), cat(idx, np.int32), cat(d2, np.float32)


def _check_radius(g, which, pts, q, radius):
    off, idx, d2 = g.radiusSearch(q, radius, which=which)
    roff, ridx, rd2 = _radius_ref(pts, q, radius)
    assert np.array_equal(off, roff) and np.array_equal(idx, ridx) and np.array_equal(d2, rd2)
    return off, idx, d2


def _cube(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def test_radius_random_clouds_far_queries_and_ties(ng, ref_kdtree):
    rng = np.random.default_rng(11)
    a = (rng.normal(size=(5000, 3)) * [10, 8, 1.5]).astype(np.float32)
    b = (rng.normal(size=(3000, 3)) * [10, 8, 1.5]).astype(np.float32)
    q = np.concatenate([a[:150], b[:100] + np.float32(0.05), (rng.normal(size=(60, 3)) * 60).astype(np.float32)])
    g = ng.NanoGICP(); g.setInputSource(a); g.setInputTarget(b)
    for radius in (0.5, 4.0):
        off, _, _ = _check_radius(g, "source", a, q, radius)
        _check_radius(g, "target", b, q, radius)
        assert np.any(np.diff(off)[-60:] == 0)  # queries far outside: empty segments
    # after swapSourceAndTarget the indices swap roles
    g.swapSourceAndTarget()
    _check_radius(g, "source", b, q, 4.0)
    _check_radius(g, "target", a, q, 4.0)
    # the lattice with duplicates: many exactly equal d2, ordered by original index
    pts, tq = ref_kdtree["ties_pts"], ref_kdtree["ties_q"]
    t = ng.NanoGICP(); t.setInputTarget(pts); t.setInputSource(pts)
    for radius in (1.0, 3.0):
        off, idx, d2 = _check_radius(t, "target", pts, tq, radius)
        _check_radius(t, "source", pts, tq, radius)
        assert len(np.unique(d2)) < len(d2) // 4


def test_radius_edges(ng):
    pts = _cube(4000, 1)
    q = pts[:40] + np.float32(0.003)
    g = ng.NanoGICP(); g.setInputTarget(pts)
    # radius <= 0: nothing
    for radius in (0.0, -1.0):
        off, idx, d2 = g.radiusSearch(q, radius)
        assert np.all(off == 0) and idx.size == 0 and d2.size == 0
    # a radius equal to an occurring float d2 excludes that point (strict <); the next float up includes it
    d = _d2_rows(pts, q[:1])[0]
    v = np.sort(d)[7]
    _, idx, d2 = _check_radius(g, "target", pts, q[:1], float(v))
    assert v not in d2 and np.all(d2 < v)
    up = float(np.nextafter(v, np.float32(np.inf)))
    _, idx_up, d2_up = _check_radius(g, "target", pts, q[:1], up)
    assert v in d2_up and len(idx_up) == len(idx) + int((d == v).sum())
    # nq = 0
    off, idx, d2 = g.radiusSearch(np.empty((0, 3), np.float32), 0.1)
    assert off.tolist() == [0] and idx.size == 0
    # capacity < total
    qq = np.ascontiguousarray(q, np.float32)
    offs = np.zeros(len(qq) + 1, np.uint64); total = C.c_size_t(0)
    L, f32 = g._L, C.POINTER(C.c_float)
    assert L.ngicp_radius_search(g._h, 1, qq.ctypes.data_as(f32), len(qq), 12, 0.01, offs.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(total)) == 0
    assert total.value > 1 and int(offs[-1]) == total.value
    idx = np.empty(total.value, np.int32); d2 = np.empty(total.value, np.float32)
    assert L.ngicp_radius_fetch(g._h, idx.ctypes.data_as(C.POINTER(C.c_int)), d2.ctypes.data_as(f32), total.value - 1) == -2
    assert L.ngicp_radius_fetch(g._h, idx.ctypes.data_as(C.POINTER(C.c_int)), d2.ctypes.data_as(f32), total.value) == 0
    # bad which, bad stride, empty slot
    assert L.ngicp_radius_search(g._h, 5, qq.ctypes.data_as(f32), len(qq), 12, 0.01, offs.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(total)) == -2
    assert L.ngicp_radius_search(g._h, 1, qq.ctypes.data_as(f32), len(qq), 10, 0.01, offs.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(total)) == -2
    with pytest.raises(ng.NgicpError) as e:
        g.radiusSearch(q, 0.01, which="source")
    assert e.value.code == -3


def test_radius_short_and_long_segments(ng):
    """Segments on both sides of the wave-sort limit (kSegShort = 512 keys) and beyond 10 000 hits (the block path)."""
    pts = _cube(40_000, 2)
    g = ng.NanoGICP(); g.setInputTarget(pts); g.setInputSource(pts[::2].copy())
    ax = np.array([0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0], np.float32)
    q = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)  # centre, faces, edges, corners
    off, _, _ = _check_radius(g, "target", pts, q, 0.04)
    n = np.diff(off)
    assert np.any((n > 1) & (n <= 512)) and np.any(n > 512)
    _check_radius(g, "source", pts[::2], q, 0.04)
    off, _, _ = _check_radius(g, "target", pts, q[len(q) // 2:len(q) // 2 + 3], 0.25)
    assert np.diff(off).max() > 10_000


# ------------------------------------------------------------------ the alignment path does not move
def test_new_entries_leave_alignment_untouched(ng, c3):
    w, make = c3
    a, b = make(), make()
    assert np.array_equal(a.getFinalTransformation(), b.getFinalTransformation())
    q = w.source[::50]
    a.fitness(); a.fitness(0.25)
    a.nearestKSearch(q, 20, which="source"); a.nearestKSearch(q, 1, which="target"); a.target_knn(q, 5)
    a.radiusSearch(q, 0.25, which="target"); a.radiusSearch(q, 0.05, which="source")
    for e in (a, b):
        e._corr = e.correspondences()[0]  # (the squared distances are only defined after linearize)
        e._stats = e.stats()
    assert np.array_equal(a._corr, b._corr)
    assert a._stats["n_src"] == b._stats["n_src"] and a._stats["passes"] == b._stats["passes"]
    a.align(w.guess); b.align(w.guess)
    assert np.array_equal(a.getFinalTransformation(), b.getFinalTransformation())
    assert a.nr_iterations_ == b.nr_iterations_
    assert np.array_equal(a.correspondences()[0], b.correspondences()[0])
