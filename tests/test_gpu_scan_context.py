"""Scan context on the GPU (ngicp_scan_context_*; k_sc_build / k_sc_norms / k_sc_match / k_sc_topk in csrc/ngicp_scan_context.h) against
the numpy model of its definition (tests/_scan_context_model.py, which proves itself - and the fixtures used here - in
test_scan_context_model_cpu.py).  The model is fed the ENGINE's tables (scanContextTables), as the definition says.

Tolerances: descriptors np.array_equal; shifts, ids and the top-k order equal; distances within 1e-9 absolute (they lie in [0, 1]), the
project's tolerance for double-valued results.  No candidate is exempted: before the engine is looked at, the match tests assert that
in the MODEL every candidate's two smallest d_k and every two neighbouring ranked distances differ by more than 1e-6, so that 1e-9 cannot
change a shift or a rank.  The exact tie is covered by the all-columns-equal descriptor.  Slot and host-descriptor queries, ranges and
single-candidate calls, and the shim are compared bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import _scan_context_cases as cs
import _scan_context_model as scm
from direct_lidar_odometry_amd import clouds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -2, -3
F = np.float32
N_DB = 70        # more than one block's worth of waves (4 per block), and no multiple of it
QUERIES = (5, 33, 60)


@pytest.fixture(scope="module")
def ng(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    return nano_gicp


@pytest.fixture()
def g(ng):
    return ng.NanoGICP()


def _raises(ng, code, fn, *a, **kw):
    with pytest.raises(ng.NgicpError) as e:
        fn(*a, **kw)
    assert e.value.code == code, f"{e.value}"


def _load(g, pts, slot):
    pts = np.ascontiguousarray(pts, dtype=F)
    if slot == 0:
        g.setInputSource(pts)
    elif slot == 1:
        g.setInputTarget(pts)
    else:
        out = g.preprocessScan(pts, remove_nan=False)
        assert len(out) == len(pts)  # nothing filtered: the slot holds the rows as given


def _model(g, pts):
    E2, b = g.scanContextTables()
    return scm.descriptor(np.asarray(pts, dtype=F), E2, b, g.getScanContextParams()[3])


def _check(g, pts, slots=(0, 1, 2), label=""):
    want = _model(g, pts)
    for slot in slots:
        _load(g, pts, slot)
        got = g.computeScanContext(slot)
        assert got.dtype == F and got.shape == want.shape
        assert np.array_equal(got, want), f"{label} slot {slot}: {np.argwhere(got != want)[:5].tolist()}"
    return want


# ---- parameters and tables ----

def test_defaults_tables_and_refused_parameters(ng, g):
    assert g.getScanContextParams() == (20, 60, F(80.0), F(2.0))
    E2, b = g.scanContextTables()
    mE2, mb = scm.tables(20, 60, 80.0)
    assert np.array_equal(E2, mE2)                 # plain arithmetic: bit for bit
    assert np.abs(b - mb).max() <= 2.0 ** -23      # cos / sin come from each side's libm: within a float step of 1
    assert b[0, 0] == 1.0 and b[0, 1] == 0.0
    g.addScanContextDescriptor(np.ones((20, 60), dtype=F))
    for bad in ((0, 60, 80.0, 2.0), (65, 60, 80.0, 2.0), (20, 0, 80.0, 2.0), (20, 61, 80.0, 2.0), (20, 66, 80.0, 2.0), (20, 60, 0.0, 2.0),
                (20, 60, -1.0, 2.0), (20, 60, np.inf, 2.0), (20, 60, np.nan, 2.0), (20, 60, 80.0, np.nan), (20, 60, 80.0, np.inf)):
        _raises(ng, ERR_ARG, g.setScanContextParams, *bad)
        assert g.getScanContextParams() == (20, 60, F(80.0), F(2.0)) and g.numScanContexts() == 1, bad  # a refused value changes nothing
    g.setScanContextParams(20, 60, 80.0, 2.0)      # the values in force: not a change
    assert g.numScanContexts() == 1
    g.setScanContextParams(20, 60, 80.0, 1.5)      # a change clears the database
    assert g.numScanContexts() == 0 and g.getScanContextParams() == (20, 60, F(80.0), F(1.5))
    g.setScanContextParams(7, 12, 30.0, 1.5)
    E2, b = g.scanContextTables()
    assert E2.shape == (8,) and b.shape == (6, 2) and np.array_equal(E2, scm.tables(7, 12, 30.0)[0])
    assert g.addScanContextDescriptor(np.zeros((7, 12), dtype=F)) == 0


# ---- descriptors ----

def test_a_scan_in_all_three_slots(g):
    scan = cs.drive_scans(12)[2]
    assert scan.shape == (3008, 3)
    D = _check(g, scan)
    assert (D > 0).sum() > 150  # (the fixture fills a good part of the descriptor)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_clouds(g, n):
    _check(g, cs.drive_scans(12)[5][:n * 11:11], label=f"n {n}")


def test_edge_points(g):
    """every rule of the definition at its edge, in one cloud per slot; the non-finite rows only where a slot takes them"""
    _, b = g.scanContextTables()
    on_boundaries = np.concatenate([np.c_[b * F(4.0), np.full(30, 1.0, F)], np.c_[b * F(-8.0), np.full(30, 0.5, F)],
                                    np.c_[b * F(0.5), np.full(30, 0.25, F)]])  # power-of-two multiples of b_k: the cross product is exactly 0
    pts = np.concatenate([on_boundaries, np.array([
        [4.0, 0.0, 0.0], [0.0, 8.0, 1.0], [-12.0, 0.0, 2.0], [0.0, -76.0, 3.0],  # r2 exactly on a ring edge: the outer ring
        [-5.0, 0.0, 1.0], [-0.0, 0.0, 0.5], [5.0, -0.0, 0.75],                    # y == 0 with x < 0; zeros of either sign
        [0.0, 0.0, 0.25],                                                        # the origin
        [80.0, 0.0, 9.0], [0.0, -80.0, 9.0], [100.0, 3.0, 9.0], [60.0, 60.0, 9.0],  # range >= L
        [79.99, 0.0, 4.0],                                                       # just inside
        [9.0, 9.0, -2.0], [9.0, 9.0, -3.0], [9.5, 9.0, -2.0],  # z + z0 <= 0 leaves the cell at 0
        [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.5], [1.0, 1.0, 1.5],      # duplicates
    ], dtype=F)])
    want = _check(g, pts, label="edges")
    assert want[1, 0] == 3.0 and want[2, 15] == 3.0 and want[3, 30] == 4.0 and want[19, 45] == 5.0  # the edge points sit in the outer ring
    # rows only the preprocessed slot takes (no index is built there): non-finite ones, a square that overflows, a height far below
    bad = np.array([[np.nan, 1.0, 50.0], [1.0, np.inf, 50.0], [1.0, 1.0, np.nan], [-np.inf, 1.0, 50.0], [2.0, 2.0, np.inf], [np.nan] * 3,
                    [3e19, 3e19, 9.0], [30.0, -7.0, -3e38]], dtype=F)
    both = np.concatenate([pts[:40], bad, pts[40:]])
    assert np.array_equal(_check(g, both, slots=(2,), label="non-finite rows"), want)
    _load(g, bad, 2)  # every point skipped: the all-zero descriptor, not an error
    assert np.array_equal(g.computeScanContext(2), np.zeros((20, 60), dtype=F))
    far = np.array([[90.0, 0.0, 1.0], [0.0, 200.0, 1.0]], dtype=F)
    assert not _check(g, far, label="all out of range").any()


def test_all_points_in_one_cell(g):
    rng = np.random.default_rng(3)
    ang, rad = rng.uniform(np.radians(12.5), np.radians(17.5), 700), rng.uniform(8.5, 11.5, 700)  # ring 2, sector 2
    pts = np.c_[rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1.0, 3.0, 700)].astype(F)
    D = _check(g, pts, label="one cell")
    assert (D > 0).sum() == 1 and D[2, 2] == (pts[:, 2] + F(2.0)).max()


@pytest.mark.parametrize("R,S,L,z0", [(1, 2, 30.0, 2.0), (64, 64, 25.0, 1.75), (20, 60, 80.0, 2.0), (3, 4, 12.5, -0.5)])
def test_parameter_extremes(g, R, S, L, z0):
    g.setScanContextParams(R, S, L, z0)
    D = _check(g, cs.drive_scans(12)[7], label=f"{R} x {S}")
    assert D.shape == (R, S) and D.any()
    _check(g, cs.drive_scans(12)[7][:65], slots=(2,), label=f"{R} x {S}, 65 points")


# ---- the database ----

def test_add_is_compute_then_add_descriptor(g):
    scans = cs.drive_scans(12)
    for i in (0, 1):
        _load(g, scans[i], 0)
        assert g.addScanContext(0) == 2 * i
        assert g.addScanContextDescriptor(g.computeScanContext(0)) == 2 * i + 1
    _load(g, scans[4], 1); assert g.addScanContext(1) == 4
    _load(g, scans[6], 2); assert g.addScanContext("preprocessed") == 5
    assert g.numScanContexts() == 6
    for i in (0, 1):
        assert g.scanContext(2 * i).tobytes() == g.scanContext(2 * i + 1).tobytes() == _model(g, scans[i]).tobytes()
    assert np.array_equal(g.scanContext(4), _model(g, scans[4])) and np.array_equal(g.scanContext(5), _model(g, scans[6]))
    # the norms too: a pair of entries is at the same distance from any query, bit for bit
    dist, shift = g.scanContextDistances(_model(g, scans[3]), 0, 4)
    assert dist[0] == dist[1] and dist[2] == dist[3] and shift[0] == shift[1] and shift[2] == shift[3]
    g.clearScanContexts()
    assert g.numScanContexts() == 0
    assert g.addScanContextDescriptor(np.zeros((20, 60), dtype=F)) == 0  # ids start again


def test_the_database_grows_past_its_first_allocation(g):
    g.setScanContextParams(2, 4, 10.0, 0.0)
    descs = [np.full((2, 4), i + 1, dtype=F) * np.arange(1, 5, dtype=F) for i in range(130)]
    for i, d in enumerate(descs):
        assert g.addScanContextDescriptor(d) == i
    for i in (0, 63, 64, 127, 128, 129):
        assert np.array_equal(g.scanContext(i), descs[i])


def test_errors_and_refused_calls_change_nothing(ng, g):
    D = _model(g, cs.drive_scans(12)[0])
    # no cloud yet: the state errors of the range select
    for slot in (0, 1, 2):
        _raises(ng, ERR_STATE, g.computeScanContext, slot)
        _raises(ng, ERR_STATE, g.addScanContext, slot)
        _raises(ng, ERR_STATE, g.scanContextDistances, slot, 0, 0)
        _raises(ng, ERR_STATE, g.matchScanContext, slot, 0, 0, 1)
    for slot in (-1, 3, 17):
        _raises(ng, ERR_ARG, g.computeScanContext, slot)
        _raises(ng, ERR_ARG, g.addScanContext, slot)
    _raises(ng, ERR_ARG, g.computeScanContext, "submap")
    assert g.numScanContexts() == 0
    for i in range(3):
        g.addScanContextDescriptor(D * F(i + 1))
    snapshot = [g.scanContext(i).copy() for i in range(3)]
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-30):
        E = D.copy(); E[7, 11] = bad
        _raises(ng, ERR_ARG, g.addScanContextDescriptor, E)
        _raises(ng, ERR_ARG, g.scanContextDistances, E, 0, 3)
        _raises(ng, ERR_ARG, g.matchScanContext, E, 0, 3, 1)
    _raises(ng, ERR_ARG, g.addScanContextDescriptor, np.zeros((20, 59), dtype=F))
    _raises(ng, ERR_ARG, g.scanContext, 3)
    _raises(ng, ERR_ARG, g.scanContext, -1)
    for begin, end in ((0, 4), (2, 1), (4, 4), (-1, 2)):
        _raises(ng, ERR_ARG, g.scanContextDistances, D, begin, end)
        _raises(ng, ERR_ARG, g.matchScanContext, D, begin, end, 1)
    for k in (0, -1, 65):
        _raises(ng, ERR_ARG, g.matchScanContext, D, 0, 3, k)
    # the C entry itself: a slot AND a descriptor, neither, null outputs
    import ctypes as C
    L, h = g._L, g._h
    fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
    d32 = np.ascontiguousarray(D); dist = np.zeros(64); ids = np.zeros(64, np.int32); shift = np.zeros(64, np.int32); n = C.c_size_t(99)
    pd, pdist, pids, pshift = d32.ctypes.data_as(fp), dist.ctypes.data_as(dp), ids.ctypes.data_as(ip), shift.ctypes.data_as(ip)
    _load(g, cs.drive_scans(12)[0], 0)
    assert L.ngicp_scan_context_distances(h, 0, pd, 0, 3, pdist, pshift) == ERR_ARG
    assert L.ngicp_scan_context_distances(h, -1, None, 0, 3, pdist, pshift) == ERR_ARG
    assert L.ngicp_scan_context_distances(h, -2, pd, 0, 3, pdist, pshift) == ERR_ARG
    assert L.ngicp_scan_context_distances(h, -1, pd, 0, 3, None, pshift) == ERR_ARG
    assert L.ngicp_scan_context_match(h, -1, pd, 0, 3, 2, pids, pdist, pshift, None) == ERR_ARG
    assert L.ngicp_scan_context_match(h, -1, pd, 0, 3, 2, None, pdist, pshift, C.byref(n)) == ERR_ARG
    assert L.ngicp_scan_context_compute(h, 0, None) == ERR_ARG and L.ngicp_scan_context_add(h, 0, None) == ERR_ARG
    assert L.ngicp_scan_context_get(h, 0, None) == ERR_ARG and L.ngicp_scan_context_tables(h, None, None) == ERR_ARG
    assert L.ngicp_scan_context_count(h, None) == ERR_ARG and L.ngicp_scan_context_kernel_ms(h, None) == ERR_ARG
    assert g.numScanContexts() == 3 and all(np.array_equal(g.scanContext(i), snapshot[i]) for i in range(3))
    assert (dist == 0).all() and (ids == 0).all() and (shift == 0).all()  # nothing was written by a refused call
    # and the accepted calls still work
    assert len(g.scanContextDistances(0, 0, 3)[0]) == 3 and g.scanContextKernelMs() > 0.0


# ---- matching ----

@pytest.fixture(scope="module")
def world(ng):
    """70 entries added from the device, three yawed revisits, and the model's table of d_k per query, computed once"""
    g = ng.NanoGICP()
    E2, b = g.scanContextTables()
    scans = cs.drive_scans(N_DB)
    model_db = [scm.descriptor(s, E2, b) for s in scans]
    for i, s in enumerate(scans):
        g.setInputSource(s)
        assert g.addScanContext(0) == i
    queries = {}
    for i in QUERIES:
        scan, _ = cs.revisit(i, N_DB)
        Q = scm.descriptor(scan, E2, b)
        dk = np.stack([scm.shift_distances(Q, C) for C in model_db])  # [entry][shift]
        queries[i] = {"scan": scan, "Q": Q, "dk": dk, "dist": dk.min(axis=1), "shift": dk.argmin(axis=1).astype(np.int32)}  # argmin: the smallest k
    return {"g": g, "db": model_db, "queries": queries}


def _assert_margins(dk, dist):
    """in the model: every candidate's two smallest d_k, and neighbouring ranked distances, differ by more than MARGIN"""
    two = np.sort(dk, axis=1)[:, :2]
    assert (two[:, 1] - two[:, 0] > cs.MARGIN).all(), "a candidate's best shift is not separated in the model"
    if len(dist) > 1:
        assert (np.diff(np.sort(dist)) > cs.MARGIN).all(), "two ranked distances are not separated in the model"


def test_the_database_holds_the_model_s_descriptors(world):
    g = world["g"]
    assert g.numScanContexts() == N_DB
    for i in range(N_DB):
        assert np.array_equal(g.scanContext(i), world["db"][i]), i


@pytest.mark.parametrize("qi", QUERIES)
def test_distances_shifts_and_ranking_of_70_entries(world, qi):
    g, q = world["g"], world["queries"][qi]
    _assert_margins(q["dk"], q["dist"])
    g.setInputSource(q["scan"])
    assert np.array_equal(g.computeScanContext(0), q["Q"])
    dist, shift = g.scanContextDistances(0, 0, N_DB)
    print(f"query {qi}: largest distance error {np.abs(dist - q['dist']).max():.3e}, bit-equal {np.array_equal(dist, q['dist'])}")
    assert dist.dtype == np.float64 and shift.dtype == np.int32
    assert np.array_equal(shift, q["shift"])
    assert (np.abs(dist - q["dist"]) <= 1e-9).all()
    order = scm.ranking(q["dist"])
    assert order[0] == qi  # the place is found (a property of the fixture, shown on the model)
    for top_k in (1, 8, 64):
        ids, d, s = g.matchScanContext(0, 0, N_DB, top_k)
        assert ids.tolist() == order[:top_k].tolist(), top_k
        assert d.tobytes() == dist[order[:top_k]].tobytes() and np.array_equal(s, shift[order[:top_k]])
    # a host descriptor is the same query, bit for bit
    dist2, shift2 = g.scanContextDistances(q["Q"], 0, N_DB)
    assert dist2.tobytes() == dist.tobytes() and np.array_equal(shift2, shift)
    m0, m1 = g.matchScanContext(0, 0, N_DB, 8), g.matchScanContext(q["Q"], 0, N_DB, 8)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m0, m1))


def test_ranges_single_candidates_and_top_k_beyond_the_range(world):
    g, q = world["g"], world["queries"][33]
    full_d, full_s = g.scanContextDistances(q["Q"], 0, N_DB)
    for a, b in ((0, 1), (3, 8), (4, 69), (17, 70), (69, 70), (31, 36)):
        _assert_margins(q["dk"][a:b], q["dist"][a:b])
        d, s = g.scanContextDistances(q["Q"], a, b)
        assert d.tobytes() == full_d[a:b].tobytes() and np.array_equal(s, full_s[a:b]), (a, b)  # an entry's values do not depend on the range
        want = scm.ranking(q["dist"][a:b], first=a)
        for top_k in (1, 3, 64):
            ids, md, ms = g.matchScanContext(q["Q"], a, b, top_k)
            assert ids.tolist() == want[:top_k].tolist() and len(ids) == min(top_k, b - a), (a, b, top_k)
            assert md.tobytes() == full_d[ids].tobytes() and np.array_equal(ms, full_s[ids])
    for e in range(N_DB):  # entry e of the whole call is the single-candidate call, bit for bit
        d, s = g.scanContextDistances(q["Q"], e, e + 1)
        assert d[0] == full_d[e] and s[0] == full_s[e], e
    for a in (0, 35, 70):  # an empty range: nothing, and success
        d, s = g.scanContextDistances(q["Q"], a, a)
        ids, md, ms = g.matchScanContext(q["Q"], a, a, 5)
        assert len(d) == len(s) == len(ids) == len(md) == len(ms) == 0
    assert len(g.scanContextDistances(q["Q"])[0]) == N_DB and len(g.matchScanContext(q["Q"], top_k=2)[0]) == 2  # the defaults: every entry


def test_ties_self_matches_and_empty_descriptors(g):
    col = np.arange(1, 21, dtype=F) * F(0.25)
    equal = np.repeat(col[:, None], 60, axis=1)
    scan = _model(g, cs.drive_scans(12)[1])
    zero = np.zeros((20, 60), dtype=F)
    for d in (equal, scan, zero, equal, np.roll(scan, 7, axis=1)):
        g.addScanContextDescriptor(d)
    dist, shift = g.scanContextDistances(equal, 0, 5)
    assert shift[0] == 0 and shift[3] == 0 and dist[0] == dist[3]  # tied at every shift: shift 0
    assert abs(dist[0]) <= 1e-12
    assert dist[2] == 1.0 and shift[2] == 0                                                        # an empty candidate
    ids, d, s = g.matchScanContext(equal, 0, 5, 2)
    assert ids.tolist() == [0, 3] and d[0] == d[1]                                                 # equal distances rank by id
    dist, shift = g.scanContextDistances(scan, 0, 5)
    assert shift[1] == 0 and abs(dist[1]) <= 1e-12 and shift[4] == 7 and abs(dist[4]) <= 1e-12     # itself at 0; rolled by 7 columns at 7
    dist, shift = g.scanContextDistances(zero, 0, 5)
    assert (dist == 1.0).all() and (shift == 0).all()                                              # an empty query
    assert g.matchScanContext(zero, 0, 5, 64)[0].tolist() == [0, 1, 2, 3, 4]
    # one entry
    g.clearScanContexts()
    g.addScanContextDescriptor(scan)
    ids, d, s = g.matchScanContext(np.roll(scan, -3, axis=1), 0, 1, 8)
    assert ids.tolist() == [0] and s.tolist() == [3] and abs(d[0]) <= 1e-12


def test_other_layouts_match_the_model(g):
    """the match kernel with fewer waves per block (64 x 64) and with one-lane and two-lane shift sets"""
    rng = np.random.default_rng(11)
    for R, S in ((64, 64), (1, 2), (5, 34)):
        g.setScanContextParams(R, S, 40.0, 2.0)
        db = [np.where(rng.random((R, S)) < 0.7, rng.integers(1, 64, (R, S)) * 0.125, 0.0).astype(F) for _ in range(9)]
        for d in db:
            g.addScanContextDescriptor(d)
        Q = np.where(rng.random((R, S)) < 0.7, rng.integers(1, 64, (R, S)) * 0.125, 0.0).astype(F)
        dk = np.stack([scm.shift_distances(Q, C) for C in db])
        two = np.sort(dk, axis=1)[:, :2]
        clear = two[:, 1] - two[:, 0] > cs.MARGIN  # (random cells, and at S = 2 exact ties: only a separated minimum fixes the shift)
        dist, shift = g.scanContextDistances(Q, 0, 9)
        assert clear.any() or S == 2
        assert np.array_equal(shift[clear], dk.argmin(axis=1)[clear]), (R, S)
        assert (np.abs(dk[np.arange(9), shift] - dk.min(axis=1)) <= 1e-9).all(), (R, S)
        assert (np.abs(dist - dk.min(axis=1)) <= 1e-9).all(), (R, S)


# ---- no side effects ----

def test_the_new_calls_leave_an_alignment_s_results_alone(g):
    scans = cs.drive_scans(12)
    q, T = cs.revisit(4, 12)
    g.preprocessScan(scans[9], remove_nan=False)
    g.setInputSource(q); g.setInputTarget(scans[4])
    guesses = np.stack([T, scm.guess(6)]).astype(F)

    def every_new_call():
        g.setScanContextParams(10, 20, 40.0, 1.0)  # a change (the database starts again), an entry of that size, and back
        g.addScanContext(0)
        g.setScanContextParams(20, 60, 80.0, 2.0)
        D = g.computeScanContext(0)
        g.computeScanContext(1); g.computeScanContext(2)
        g.addScanContext(0); g.addScanContext(1); g.addScanContext(2); g.addScanContextDescriptor(D)
        g.scanContext(1); g.numScanContexts(); g.scanContextTables(); g.getScanContextParams(); g.scanContextKernelMs()
        g.scanContextDistances(0); g.scanContextDistances(D); g.matchScanContext(2, top_k=3); g.matchScanContext(D, top_k=64)
        g.scanContextGuess(5)
        g.clearScanContexts()

    every_new_call()  # (the workspace exists from here on: stats()["device_allocs"] stays)
    g.alignBatch(guesses)
    lanes = [g.lm_trace(lane=i).copy() for i in range(2)]
    g.align(T)
    g.linearize(T.astype(np.float64))
    e0 = g.compute_error(T.astype(np.float64))

    def state():
        return (g.getFinalTransformation().copy(), g.getFinalHessian().copy(), g.nr_iterations_, g.converged_, g.lm_trace().copy(), g.correspondences(), g.stats())

    before = state()
    every_new_call()
    after = state()
    for a, b in zip(before, after):
        if isinstance(a, tuple):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b)
        else:
            assert a == b
    for i, tr in enumerate(lanes):
        assert np.array_equal(g.lm_trace(lane=i), tr), f"lane {i} of the earlier alignBatch"
    assert g.compute_error(T.astype(np.float64)) == e0


# ---- end to end ----

def test_a_revisit_is_found_and_its_shift_starts_the_alignment(ng):
    """12 places along a drive; the query is taken at place 7 with the sensor yawed by 37 degrees and moved 0.4 m.  "The same pose": an
    alignment stops when a step moves the pose by less than the handle's transformation epsilon (translation) and rotation epsilon
    (rotation matrix entries), so each run ends within about one epsilon of the fixed point it converges to; two runs that reach the
    same fixed point therefore end within twice the epsilons of each other, and that is the bound asserted."""
    g = ng.NanoGICP()
    scans = cs.drive_scans(12)
    for i, s in enumerate(scans):
        g.setInputSource(s)
        assert g.addScanContext(0) == i
    place = 7
    q, T_true = cs.revisit(place, 12)
    g.setInputSource(q)
    ids, dist, shift = g.matchScanContext(0, 0, 12, 3)
    print(f"top-3 {ids.tolist()} at {dist.tolist()}, shifts {shift.tolist()}")
    assert ids[0] == place
    sector = cs.REVISIT_YAW_DEG / (360.0 / 60)  # 6.17
    assert abs(int(shift[0]) - round(sector)) <= 1
    guess = g.scanContextGuess(int(shift[0]))
    assert guess.dtype == F and np.array_equal(guess, scm.guess(int(shift[0])))
    g.setInputTarget(scans[place])
    g.align(guess)
    T_sc, ok_sc = g.getFinalTransformation().copy(), g.hasConverged()
    g.align(T_true.astype(F))
    T_gt, ok_gt = g.getFinalTransformation().copy(), g.hasConverged()
    dt, dr = clouds.pose_error(T_sc, T_gt)
    dt_true, dr_true = clouds.pose_error(T_gt, T_true)
    print(f"from the shift vs from the truth: {dt:.2e} m, {dr:.2e} rad; the truth's own result is {dt_true:.2e} m, {dr_true:.2e} rad from the truth")
    assert ok_sc and ok_gt
    assert dt <= 2.0 * g._p["trans_eps"] and dr <= 2.0 * g._p["rot_eps"]
    # the recipe with several guesses: the shift and its neighbours in one alignBatch, ranked by fitness
    guesses = np.stack([g.scanContextGuess(int(shift[0]) + o) for o in (-1, 0, 1)])
    Ts, conv, _, _ = g.alignBatch(guesses)
    scores, _ = g.fitnessBatch(Ts, 1.0)
    best = int(np.argmin(scores))
    assert conv[best] and clouds.pose_error(Ts[best], T_gt)[0] <= 2.0 * g._p["trans_eps"]


def test_the_shim_agrees_with_python(ng, tmp_path):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(tmp_path), "scan_context_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "scan_context_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    scans = cs.drive_scans(12)
    q, _ = cs.revisit(3, 12)
    paths = []
    for name, c in [("query", q)] + [(f"kf{i}", s) for i, s in enumerate(scans)]:
        paths.append(os.path.join(str(tmp_path), name + ".bin"))
        np.ascontiguousarray(c, dtype=F).tofile(paths[-1])
    run = subprocess.run([exe, "3"] + paths, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in run.stdout.splitlines() if not ln.startswith("added ")}
    assert [ln for ln in run.stdout.splitlines() if ln.startswith("added ")] == [f"added {i}" for i in range(12)]

    def records(tok):
        n = int(tok[0])
        return [(int(tok[1 + 3 * i]), float.fromhex(tok[2 + 3 * i]), int(tok[3 + 3 * i])) for i in range(n)]

    g = ng.NanoGICP()
    for s in scans:
        g.setInputSource(s); g.addScanContext(0)
    g.setInputSource(q)
    assert lines["params"][:2] == ["20", "60"] and float.fromhex(lines["params"][2]) == 80.0 and float.fromhex(lines["params"][3]) == 2.0
    assert lines["refused"] == ["0"] and "n_sectors" in run.stderr
    E2, b = g.scanContextTables()
    assert lines["tables"][:3] == ["1", "21", "60"] and float.fromhex(lines["tables"][3]) == E2[-1] and float.fromhex(lines["tables"][4]) == b[1, 0]
    assert lines["count"] == ["12"]
    ids, dist, shift = g.matchScanContext(0, 0, 12, 3)
    assert records(lines["match"]) == records(lines["match_desc"]) == list(zip(ids.tolist(), dist.tolist(), shift.tolist()))
    assert ids[0] == 3
    best_shift = int(shift[0])
    d_all, s_all = g.scanContextDistances(0, 0, 12)
    assert records(lines["distances"]) == list(zip(range(12), d_all.tolist(), s_all.tolist()))
    ids, dist, shift = g.matchScanContext(0, 6, 12, 3)
    assert records(lines["tail"]) == list(zip(ids.tolist(), dist.tolist(), shift.tolist()))
    assert lines["added_desc"] == ["12", "same", "1"]
    self_match = records(lines["self"])
    assert len(self_match) == 1 and self_match[0][0] == 12 and self_match[0][2] == 0 and abs(self_match[0][1]) <= 1e-12
    assert lines["bad_range"] == ["0"]
    g.setInputTarget(scans[3])
    g.align(g.scanContextGuess(best_shift))
    assert lines["aligned"][0] == str(int(g.hasConverged()))
    T = np.array([float.fromhex(t) for t in lines["aligned"][1:]], dtype=F).reshape(4, 4)
    assert np.array_equal(T, g.getFinalTransformation())
    assert lines["cleared"] == ["0"]
