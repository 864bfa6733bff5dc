"""The merged voxel map on the GPU (ngicp_set_voxel_submap_merge; k_voxel_part_fill / k_voxel_part_gather / k_voxel_merge_fill in
csrc/ngicp_voxel.h) against the numpy model of its definition (tests/_vgicp_submap_model.py, which proves itself in
test_vgicp_submap_model_cpu.py): the keyframes' parts, merged maps, the exact relations to the map summed over the points, which route a
build takes and what it caches, the refusal, whole alignments pass by pass, and what the setting must leave alone.

Tolerances are the project's for the same quantities (tests/test_gpu_vgicp.py): ijk, counts and voxel numbers exact, map entries within
1e-12 relative (bit-equality is expected and printed), per-pass y0 / yi / H within _pass_check.H_TOL."""
import numpy as np
import pytest

import _vgicp_model as vm
import _vgicp_nbr_model as nm
import _vgicp_submap_model as sm
from _pass_check import H_TOL
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


def _spd(n, seed):
    """n random symmetric positive definite 3x3 matrices as (n, 4, 4) covariances."""
    A = np.random.default_rng(seed).normal(0, 0.1, (n, 3, 3))
    out = np.zeros((n, 4, 4))
    out[:, :3, :3] = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return out


def _cube(n, half, seed, offset=(0.0, 0.0, 0.0)):
    return (np.random.default_rng(seed).uniform(-half, half, (n, 3)) + np.asarray(offset)).astype(np.float32)


def _lattice_planes(res):
    """Points exactly on lattice planes, negative ones included, some twice; and points just below a plane (tests/test_gpu_vgicp.py)."""
    k = np.arange(-6, 7, dtype=np.float32) * np.float32(res)
    p = np.stack(np.meshgrid(k, k[::3], k[::4], indexing="ij"), -1).reshape(-1, 3)
    below = np.nextafter(p[::5], np.float32(-np.inf))
    return np.ascontiguousarray(np.r_[p, p[::7], below, np.array([[-0.0, 0.0, -0.0]], np.float32)])


def _check_map(got, m, label):
    """tests/test_gpu_vgicp.py's rule: ijk and counts exact; every mean and covariance entry within 1e-12 of the model's, relative to
    that entry itself.  Both sides add the same terms in the same order in IEEE double without fused operations and divide once, so they
    are expected to agree to the bit (printed)."""
    ijk, mean, cov, cnt = got
    assert len(ijk) == len(m), f"{label}: {len(ijk)} voxels, the model has {len(m)}"
    assert np.array_equal(ijk, m.ijk) and np.array_equal(cnt, m.count), label
    dm, dc = np.abs(mean - m.mean), np.abs(cov - m.cov)
    print(f"{label}: {len(m)} voxels, largest count {m.count.max()}, mean off by {(dm / np.maximum(np.abs(m.mean), 1e-300)).max():.1e}, "
          f"cov by {(dc / np.maximum(np.abs(m.cov), 1e-300)).max():.1e} (relative), bit-equal: {np.array_equal(mean, m.mean) and np.array_equal(cov, m.cov)}")
    assert (dm <= 1e-12 * np.abs(m.mean)).all() and (dc <= 1e-12 * np.abs(m.cov)).all(), label


def _check_part(got, p, label):
    """a keyframe's part under the same rule, the sums in place of the means"""
    ijk, s, c, cnt = got
    assert len(ijk) == len(p), f"{label}: {len(ijk)} voxels, the model has {len(p)}"
    assert np.array_equal(ijk, p.ijk) and np.array_equal(cnt, p.count), label
    ds, dc = np.abs(s - p.sum), np.abs(c - p.covsum)
    print(f"{label}: {len(p)} voxels, largest count {p.count.max()}, bit-equal: {np.array_equal(s, p.sum) and np.array_equal(c, p.covsum)}")
    assert (ds <= 1e-12 * np.abs(p.sum)).all() and (dc <= 1e-12 * np.abs(p.covsum)).all(), label


class Store:
    """A handle with a keyframe store, and what the store holds per keyframe (points and covariances in original order, read back through
    a one-keyframe submap), for the model."""

    def __init__(self, ng, res=1.0):
        self.ng = ng
        self.prod, self.g = ng.NanoGICP(), ng.NanoGICP()
        self.g.setVoxelResolution(res)
        self.pts, self.covs, self._parts = [], [], {}

    def _read_back(self, kid):
        self.g.setSubmapKeyframes([kid])
        self.pts.append(self.g.targetPoints())
        self.covs.append(self.g.getTargetCovariances())
        return kid

    def add_with_covs(self, pts, covs):
        """the keyframe is the producer's source and the covariances set on it"""
        self.prod.setInputSource(pts)
        self.prod.setSourceCovariances(covs)
        kid = self._read_back(self.g.addKeyframe(self.prod))
        assert np.array_equal(self.pts[kid], pts) and np.array_equal(self.covs[kid][:, :3, :3], covs[:, :3, :3])
        return kid

    def add_scan(self, scan, pose):
        """the keyframe is the scan transformed on the device, with the engine's own covariances (k = 20)"""
        self.prod.setInputSource(scan)
        return self._read_back(self.g.addKeyframeTransformed(self.prod, pose))

    def parts(self, res):
        have = self._parts.setdefault(res, [])
        for k in range(len(have), len(self.pts)):  # (keyframes added since the last call)
            have.append(sm.VoxelPart(self.pts[k], self.covs[k], res))
        return have

    def model(self, ids, res):
        return sm.MergedVoxelMap(self.parts(res), ids)

    def close(self):
        self.prod.close(); self.g.close()


# ---- 1. the parts ---------------------------------------------------------------------------------------------------------------------
def test_keyframe_parts_match_the_model(ng):
    """1, 255, 256, 257 and 4100 points (one thread's tail, a block's edge, a radix tile and a scan tile crossed) with set covariances, and a
    VLP-16 scan with the engine's own."""
    st = Store(ng)
    for n in (1, 255, 256, 257, 4100):
        st.add_with_covs(_cube(n, 3.0 if n < 4100 else 10.0, n), _spd(n, 100 + n))
    sc = clouds.make_scene()
    st.add_scan(clouds.vlp16(sc, clouds.make_pose((0.5, 0.2, 0.0), (0, 0, 3.0)), noise_seed=51, cols=150), clouds.make_pose((0.5, 0.2, 0.0), (0, 0, 3.0)))
    for res in (1.0, 0.25):
        st.g.setVoxelResolution(res)
        for kid, p in enumerate(st.parts(res)):
            _check_part(st.g.keyframeVoxelMap(kid), p, f"keyframe {kid} ({len(st.pts[kid])} points) at {res}")
    assert len(st.parts(1.0)[4]) > 1024  # more than one block of the fill, more than a radix tile of voxels
    assert st.g.voxelMapMergeStats()["parts_built"] == 12 and st.g.voxelMapBuilds() == 0
    with pytest.raises(ng.NgicpError) as e:
        st.g.keyframeVoxelMap(6)
    assert e.value.code == -2
    st.g.setVoxelResolution(0)
    with pytest.raises(ng.NgicpError) as e:
        st.g.keyframeVoxelMap(0)
    assert e.value.code == -3
    st.close()


# ---- 2. merged maps and their exact relations to the map summed over the points -----------------------------------------------------------
def _both_maps(st, ids, res, label):
    """The map of the submap `ids` with the setting on (checked against the model) and off, on the same handle; the exact relations."""
    g = st.g
    g.setVoxelResolution(res)
    g.setVoxelSubmapMerge(True)
    g.setSubmapKeyframes(ids)
    before = g.voxelMapMergeStats()["merged_builds"]
    on = g.voxelMap()
    assert g.voxelMapMergeStats()["merged_builds"] == before + 1, f"{label}: not built by the merged route"
    m = st.model(ids, res)
    _check_map(on, m, label)
    g.setVoxelSubmapMerge(False)
    off = g.voxelMap()
    assert g.voxelMapMergeStats()["merged_builds"] == before + 1
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[3], off[3]), f"{label}: ijk or counts differ between the routes"
    same = np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2])
    print(f"{label}: means and covariances of the two routes bit-equal: {same}")
    if len(ids) == 1:
        assert same, f"{label}: one keyframe, and the two routes differ"
    return on, off, m


@pytest.fixture(scope="module")
def vlp(ng):
    """Three VLP-16 keyframes (cols = 150) at the poses of the existing submap test; shared, the store is left unchanged."""
    st = Store(ng)
    sc = clouds.make_scene()
    for i in range(3):
        pose = clouds.make_pose((0.5 * i, 0.2 * i, 0.0), (0, 0, 3.0 * i))
        st.add_scan(clouds.vlp16(sc, pose, noise_seed=50 + i, cols=150), pose)
    yield st
    st.close()


@pytest.mark.parametrize("ids", [[0, 1, 2], [0, 2], [2, 0], [1], [0, 0]], ids=lambda v: "ids_" + "_".join(map(str, v)))
def test_merged_map_of_scans_matches_the_model(vlp, ids):
    on, _, m = _both_maps(vlp, ids, 1.0, f"scans {ids}")
    assert on[3].sum() == sum(len(vlp.pts[k]) for k in ids)
    if ids == [0, 0]:
        one = vlp.model([0], 1.0)
        assert np.array_equal(on[3], 2 * one.count)


@pytest.fixture(scope="module")
def cubes(ng):
    """Three cube keyframes of about 1 400 occupied voxels each at 1 m."""
    st = Store(ng)
    for i in range(3):
        st.add_with_covs(_cube(1550, 10.0, 200 + i), _spd(1550, 210 + i))
    yield st
    st.close()


@pytest.mark.parametrize("res", [1.0, 0.25, 4.0])
def test_merged_map_of_cubes_crosses_the_tiles(cubes, res):
    parts = cubes.parts(res)
    on, _, m = _both_maps(cubes, [0, 1, 2], res, f"cubes at {res}")
    if res == 1.0:
        sizes = [len(p) for p in parts]
        assert all(1300 < s < 1500 for s in sizes), sizes
        assert sum(sizes) > 4096, "the gathered list does not cross a scan tile"
        assert len(m) > 1024, "the merged voxels do not cross a block of the scan"
    _both_maps(cubes, [2, 1], res, f"cubes [2, 1] at {res}")


def test_merged_map_of_keyframes_that_share_no_voxel_every_voxel_and_lattice_planes(ng):
    st = Store(ng)
    a = st.add_with_covs(_cube(700, 3.0, 300), _spd(700, 301))
    b = st.add_with_covs(_cube(600, 3.0, 302, offset=(100.0, -50.0, 20.0)), _spd(600, 303))
    on, _, m = _both_maps(st, [a, b], 1.0, "no shared voxel")
    assert len(m) == len(st.parts(1.0)[a]) + len(st.parts(1.0)[b])
    # every voxel shared: the same 1 000 voxels, one point each in one keyframe and two each in the other
    c = np.arange(-5, 5, dtype=np.float32) + np.float32(0.5)
    centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    jit = lambda seed, n: np.random.default_rng(seed).uniform(-0.4, 0.4, (n, 3)).astype(np.float32)
    e = st.add_with_covs(np.ascontiguousarray(centres[::-1] + jit(304, 1000)), _spd(1000, 305))
    f = st.add_with_covs(np.ascontiguousarray(np.r_[centres, centres] + jit(306, 2000)), _spd(2000, 307))
    on, _, m = _both_maps(st, [e, f], 1.0, "every voxel shared")
    assert len(m) == 1000 and (m.count == 3).all()
    # lattice planes, negative ones included, split over two keyframes
    for res in (1.0, 0.25):
        p = _lattice_planes(res)
        i = st.add_with_covs(np.ascontiguousarray(p[0::2]), _spd(len(p[0::2]), 308))
        j = st.add_with_covs(np.ascontiguousarray(p[1::2]), _spd(len(p[1::2]), 309))
        on, _, m = _both_maps(st, [i, j], res, f"lattice planes at {res}")
        assert (m.ijk < 0).any() and np.array_equal(m.ijk, vm.VoxelMap(p, _spd(len(p), 0), res).ijk)
    st.close()


# ---- 3. route and cache ------------------------------------------------------------------------------------------------------------------
def test_which_route_a_build_takes_and_what_it_caches(ng):
    st = Store(ng)
    for i in range(4):
        st.add_with_covs(_cube(900, 4.0, 400 + i), _spd(900, 410 + i))
    g = st.g
    stats = g.voxelMapMergeStats
    assert g.getVoxelSubmapMerge() is False and stats() == dict(merged_builds=0, parts_built=0, last_parts_ms=0.0, last_merge_ms=0.0)
    # the setting off: the point route
    g.setSubmapKeyframes([0, 1, 2])
    g.voxelMap()
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (0, 0, 1)
    # the setting on with a host target: still the point route
    g.setVoxelSubmapMerge(True)
    assert g.getVoxelSubmapMerge() is True
    host = np.concatenate(st.pts[:2])
    g.setInputTarget(host); g.setTargetCovariances(np.concatenate(st.covs[:2]))
    _check_map(g.voxelMap(), vm.VoxelMap(host, np.concatenate(st.covs[:2]), 1.0), "host target with the setting on")
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (0, 0, 2)
    # [0, 1, 2] and then [1, 2, 3]: four parts in all
    g.setSubmapKeyframes([0, 1, 2])
    _check_map(g.voxelMap(), st.model([0, 1, 2], 1.0), "[0, 1, 2]")
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (1, 3, 3)
    g.setSubmapKeyframes([1, 2, 3])
    _check_map(g.voxelMap(), st.model([1, 2, 3], 1.0), "[1, 2, 3]")
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (2, 4, 4)
    s = stats()
    assert s["last_parts_ms"] > 0.0 and s["last_merge_ms"] > 0.0
    # the same id list again: nothing is built
    assert g.setSubmapKeyframes([1, 2, 3]) is False
    g.voxelMap(); g.getVoxelMapSize()
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (2, 4, 4)
    # setting the value already set does nothing
    g.setVoxelSubmapMerge(True)
    g.voxelMap()
    assert g.voxelMapBuilds() == 4
    # a resolution change rebuilds the listed parts (and only those)
    g.setVoxelResolution(2.0)
    _check_map(g.voxelMap(), st.model([1, 2, 3], 2.0), "[1, 2, 3] at 2 m")
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (3, 7, 5)
    g.setSubmapKeyframes([0, 1])
    g.voxelMap()
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (4, 8, 6)
    # setTargetCovariances on the submap target: the next build takes the point route
    pts = g.targetPoints()
    ct = _spd(len(pts), 420)
    g.setTargetCovariances(ct)
    _check_map(g.voxelMap(), vm.VoxelMap(pts, ct, 2.0), "submap with other covariances")
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (4, 8, 7)
    g.calculateTargetCovariances()
    g.voxelMap()
    assert (stats()["merged_builds"], g.voxelMapBuilds()) == (4, 8)
    # a new submap has the store's covariances again: merged
    g.setSubmapKeyframes([1, 0])
    merged = g.voxelMap()
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (5, 8, 9)
    # flipping the setting rebuilds, by the other route
    g.setVoxelSubmapMerge(False)
    straight = g.voxelMap()
    assert (stats()["merged_builds"], g.voxelMapBuilds()) == (5, 10)
    assert np.array_equal(merged[0], straight[0]) and np.array_equal(merged[3], straight[3])
    g.setVoxelSubmapMerge(True)
    again = g.voxelMap()
    assert (stats()["merged_builds"], stats()["parts_built"], g.voxelMapBuilds()) == (6, 8, 11)
    for x, y in zip(merged, again):
        assert np.array_equal(x, y)
    # the setting is remembered while the voxel mode is off
    g.setVoxelResolution(0)
    assert g.getVoxelSubmapMerge() is True
    g.setVoxelResolution(2.0)
    # after clearKeyframes the parts are gone
    g.clearKeyframes()
    with pytest.raises(ng.NgicpError) as e:
        g.keyframeVoxelMap(0)
    assert e.value.code == -2
    assert stats()["parts_built"] == 8
    st.close()


# ---- 4. refusal --------------------------------------------------------------------------------------------------------------------------
def test_a_keyframe_beyond_2_pow_20_voxels_is_refused(ng):
    st = Store(ng, res=1.0)
    st.add_with_covs(_cube(100, 3.0, 500), _spd(100, 501))
    far = np.r_[_cube(100, 3.0, 502), np.array([[262144.0, 0, 0]], np.float32)]  # 2^18 m / 0.25 m = 2^20
    st.add_with_covs(far, _spd(101, 503))
    g = st.g
    g.setVoxelSubmapMerge(True)
    g.setVoxelResolution(0.25)
    g.setSubmapKeyframes([0, 1])
    with pytest.raises(ng.NgicpError) as e:
        g.voxelMap()
    assert e.value.code == -2 and "keyframe 1" in str(e.value)
    g.setInputSource(_cube(50, 3.0, 504))
    with pytest.raises(ng.NgicpError) as e:
        g.align()
    assert e.value.code == -2 and "keyframe 1" in str(e.value)
    with pytest.raises(ng.NgicpError) as e:
        g.keyframeVoxelMap(1)
    assert e.value.code == -2
    assert g.voxelMapMergeStats()["merged_builds"] == 0
    g.setVoxelResolution(1.0)  # the same keyframes at 1 m: |i| = 2^18
    _check_map(g.voxelMap(), st.model([0, 1], 1.0), "at a coarser resolution")
    g.align()
    assert g.voxelMapMergeStats()["merged_builds"] == 1
    st.close()


# ---- 5. alignment ------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@pytest.fixture(scope="module")
def s2m(ng):
    """clouds.scan_to_submap(3008, 2) rebuilt through the keyframe store (each keyframe with the engine's own covariances, k = 20); the
    model's merged maps are built once per resolution and shared."""
    w = clouds.scan_to_submap(3008, 2)
    st = Store(ng)
    off = 0
    for n in w.keyframe_sizes:
        st.prod.setInputSource(np.ascontiguousarray(w.target[off:off + n]))
        st._read_back(st.g.addKeyframe(st.prod))
        off += n
    assert np.array_equal(np.concatenate(st.pts), w.target)
    e = ng.NanoGICP()
    e.setInputSource(w.source); e.calculateSourceCovariances()
    cs = e.getSourceCovariances()
    e.close()
    yield dict(w=w, st=st, cs=cs, ct=np.concatenate(st.covs))
    st.close()


def _merged_engine(ng, s2m, K, res=1.0):
    """a fresh handle with the shared store's keyframes (the same device objects would need the same handle: they are added again)"""
    w, st = s2m["w"], s2m["st"]
    g = ng.NanoGICP()
    g.setVoxelResolution(res)
    g.setNeighborSearchMethod(K)
    g.setVoxelSubmapMerge(True)
    for p, c in zip(st.pts, st.covs):  # the store's points and covariances, set: the model's map and this handle's come from the same numbers
        st.prod.setInputSource(p)
        st.prod.setSourceCovariances(c)
        g.addKeyframe(st.prod)
    g.setSubmapKeyframes(list(range(len(st.pts))))
    g.setInputSource(w.source); g.setSourceCovariances(s2m["cs"])
    return g


def _merged_model(s2m, K, res=1.0):
    w, st = s2m["w"], s2m["st"]
    m = nm.VoxelGICPNbrModel.__new__(nm.VoxelGICPNbrModel)
    vm.NumpyGICP.__init__(m, w.source, w.target, s2m["cs"], s2m["ct"])
    m.vmap = st.model(list(range(len(st.pts))), res)
    m.set_neighbors(K)
    return m


@pytest.mark.parametrize("K", [1, 7])
def test_every_pass_of_an_alignment_on_the_merged_map_matches_the_model(ng, s2m, K):
    """tests/test_gpu_vgicp.py's method (LM, the defaults) with the model on the MERGED model map: align(max_iter = k) for every k up to the
    full run; at the pose of every trace row's linearisation the (n, K) voxel numbers are exact, y0 / yi / H within H_TOL."""
    w = s2m["w"]
    g, m = _merged_engine(ng, s2m, K), _merged_model(s2m, K)
    guess = np.asarray(w.guess, np.float32)
    g.align(guess)
    assert g.voxelMapMergeStats()["merged_builds"] == 1
    full = (g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), g.nr_iterations_, g.converged_)
    n_full = g.nr_iterations_ + 1
    start, end = clouds.pose_error(guess, w.gt), clouds.pose_error(full[0], w.gt)
    print(f"DIRECT{K}: {n_full} iterations, converged {g.converged_}, pose error {start[0]:.4f} m / {start[1]:.5f} rad -> {end[0]:.4f} m / {end[1]:.5f} rad")
    poses, H_at = [guess], {}
    Hg = full[2]
    for k in range(1, n_full + 1):
        where = f"DIRECT{K}: pass {k} of {n_full}"
        g.setMaximumIterations(k)
        g.align(guess)
        T, Hg, tr = g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.lm_trace().copy()
        cn = g.voxel_correspondences()
        corr, sqd = g.correspondences()
        Hm, _, em = m.linearize(poses[k - 1].astype(np.float64))
        assert np.array_equal(cn, m.corr_n), f"{where}: voxel numbers differ at {np.argwhere(cn != m.corr_n)[:5].tolist()}"
        assert np.array_equal(corr, m.corr) and np.array_equal(sqd, m.sqd), where
        H_at[k - 1] = Hm
        rows = tr[tr[:, 0] == k - 1] if len(tr) else tr
        dE = 0.0
        for y0 in rows[:, 2] if len(rows) else []:
            dE = max(dE, _rel(y0, em))
            assert _rel(y0, em) <= H_TOL, f"{where}: y0 {y0!r} vs the model's {em!r}"
        if len(rows) and rows[-1, 7] == 1:
            yo = m.compute_error(T.astype(np.float64))
            dE = max(dE, _rel(rows[-1, 3], yo))
            assert _rel(rows[-1, 3], yo) <= H_TOL, f"{where}: yi {rows[-1, 3]!r} of the accepted trial vs the model's {yo!r}"
        if len(tr) and tr[-1, 7] == 0:  # ended on a rejected trial: the pose stayed, H is that of the last accepted step
            assert np.array_equal(T, poses[k - 1]), f"{where}: a rejected trial moved the pose"
            n_acc = int(tr[:, 7].sum())
            Href = H_at[n_acc - 1] if n_acc else np.eye(6)
        else:
            Href = Hm
        dH = float(np.abs(Hg - Href).max() / np.abs(Href).max())
        print(f"{where}: pairs per point {(cn >= 0).mean() * cn.shape[1]:.3f}, |dH|/|H| {dH:.1e}, y0/yi rel. {dE:.1e}")
        assert dH <= H_TOL, f"{where}: |dH|/|H| = {dH:.2e}"
        n_rows = int(np.sum(full[1][:, 0] < k)) if len(full[1]) else 0
        assert tr.shape == (n_rows, 8) and np.array_equal(tr, full[1][:n_rows]), f"{where}: the LM trace is not a prefix of the full run's"
        poses.append(T)
    assert np.array_equal(poses[-1], full[0]) and np.array_equal(Hg, full[2]) and (g.nr_iterations_, g.converged_) == full[3:]
    assert g.voxelMapMergeStats()["merged_builds"] == 1 and g.voxelMapBuilds() == 1  # one map for all of it
    assert end[0] < start[0] and end[1] < start[1]
    g.close()


@pytest.mark.parametrize("K", [1, 7])
def test_batch_lanes_on_the_merged_map_equal_single_alignments(ng, s2m, K):
    w = s2m["w"]
    g = _merged_engine(ng, s2m, K)
    guesses = np.stack([np.asarray(w.guess, np.float32), np.eye(4, dtype=np.float32),
                        (w.gt @ clouds.make_pose((0.1, 0.05, -0.02), (0.5, 0.2, -1.0))).astype(np.float32)])
    T, conv, nit, H = g.alignBatchVoxel(guesses)
    assert g.voxelMapMergeStats()["merged_builds"] == 1 and g.voxelMapBuilds() == 1
    for lane, guess in enumerate(guesses):
        g.align(guess)
        assert np.array_equal(T[lane], g.getFinalTransformation()) and np.array_equal(H[lane], g.getFinalHessian()), f"lane {lane}"
        assert (bool(conv[lane]), int(nit[lane])) == (bool(g.converged_), g.nr_iterations_), f"lane {lane}"
    assert g.voxelMapBuilds() == 1
    g.close()


# ---- 6. hygiene --------------------------------------------------------------------------------------------------------------------------
def test_the_setting_off_after_having_been_on_leaves_nothing_behind(ng, s2m):
    w = s2m["w"]

    def outcome(g):
        g.align(w.guess)
        return (*g.voxelMap(), g.getFinalTransformation().copy(), g.lm_trace().copy(), g.getFinalHessian().copy(), g.correspondences()[0])

    g = _merged_engine(ng, s2m, 1)
    on = outcome(g)
    g.setVoxelSubmapMerge(False)
    with pytest.raises(ng.NgicpError):  # the correspondences went with the map they number
        g.correspondences()
    off = outcome(g)
    fresh = _merged_engine(ng, s2m, 1)
    fresh.setVoxelSubmapMerge(False)
    want = outcome(fresh)
    assert fresh.voxelMapMergeStats() == dict(merged_builds=0, parts_built=0, last_parts_ms=0.0, last_merge_ms=0.0)
    for a, b in zip(off, want):
        assert np.array_equal(a, b)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[3], off[3])
    print(f"final pose with the setting on and off: equal {np.array_equal(on[4], off[4])}, "
          f"apart by {np.abs(on[4].astype(np.float64) - off[4]).max():.2e}")
    g.close(); fresh.close()
