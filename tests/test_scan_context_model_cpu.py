"""The numpy restatement of the scan context definition (tests/_scan_context_model.py) against hand-computed cells and against the
properties the definition promises, and the fixtures of tests/test_gpu_scan_context.py against the margins that test relies on.  No GPU."""
import numpy as np

import _scan_context_cases as cs
import _scan_context_model as scm

F = np.float32


def test_tables_are_the_header_s():
    E2, b = scm.tables(4, 8, 8.0)
    assert E2.dtype == F and b.dtype == F
    assert np.array_equal(E2, np.array([0, 4, 16, 36, 64], dtype=F))  # edges 0, 2, 4, 6, 8
    assert b.shape == (4, 2)
    assert np.array_equal(b[0], np.array([1, 0], dtype=F))
    assert b[2, 1] == F(1.0) and abs(float(b[2, 0])) < 1e-7  # 90 degrees: (float)cos(pi / 2) is tiny, not 0
    assert b[1, 0] == b[1, 1] or abs(float(b[1, 0]) - float(b[1, 1])) < 1e-7


def test_hand_computed_cells():
    E2, b = scm.tables(4, 8, 8.0)  # rings 2 m wide, sectors of 45 degrees
    pts = np.array([
        [1.0, 0.5, 0.0],      # r2 1.25 -> ring 0; 26.6 degrees -> sector 0; v 2
        [0.5, 1.0, 1.0],      # 63.4 degrees -> sector 1; v 3
        [-3.0, 0.1, -1.0],    # r2 9.01 -> ring 1; 178 degrees -> sector 3; v 1
        [-3.0, -0.1, 0.5],    # low; mirrored to (3, 0.1): sector 0 + 4; ring 1; v 2.5
        [0.0, -5.0, 2.0],     # low; mirrored to (0, 5): 90 degrees sits ON boundary 2 -> passed boundaries 1, 2 -> sector 2 + 4; ring 2; v 4
        [2.0, 0.0, 0.0],      # r2 == E2_1 exactly -> the outer ring 1; sector 0
        [-2.0, 0.0, 1.5],     # y == 0, x < 0 -> low, mirrored to (2, 0): sector 4; ring 1; v 3.5
        [8.0, 0.0, 5.0],      # r2 == E2_R -> skipped
        [1.0, 0.5, -2.0],     # v == 0: leaves the cell alone
        [1.0, 0.5, -7.0],     # v < 0: leaves the cell alone
        [np.nan, 0.0, 9.0], [0.0, np.inf, 9.0], [1.0, 1.0, -np.inf],  # skipped
        [0.0, 0.0, 0.25],     # the origin: ring 0, not low, every cross product is 0 -> sector 3; v 2.25
    ], dtype=F)
    want = np.zeros((4, 8), dtype=F)
    want[0, 0], want[0, 1], want[1, 3], want[1, 4], want[2, 6], want[1, 0], want[0, 3] = 2.0, 3.0, 1.0, 3.5, 4.0, 2.0, 2.25
    D = scm.descriptor(pts, E2, b)
    assert D.dtype == F and np.array_equal(D, want), D
    assert np.array_equal(scm.norms(D)[:2], np.array([np.sqrt(8.0), 3.0]))


def test_hand_computed_distance():
    Q = np.zeros((2, 4), dtype=F)
    C = np.zeros((2, 4), dtype=F)
    Q[:, 0], Q[:, 1] = (3, 4), (1, 0)
    C[:, 1], C[:, 2] = (3, 4), (0, 2)   # Q's column 0 sits on C's column 1; Q's column 1 on C's column 2, orthogonal to it
    d = scm.shift_distances(Q, C)
    assert d[1] == 1.0 - (25.0 / 25.0 + 0.0 / 2.0) / 2.0  # two counted columns: one aligned, one orthogonal
    assert d[0] == 1.0 - ((1 * 3 + 0 * 4) / (1.0 * 5.0)) / 1.0  # shift 0: only Q's column 1 meets a non-empty column (C's column 1)
    assert d[3] == 1.0  # no non-empty column meets one
    assert scm.distance(Q, C) == (float(d.min()), int(np.argmin(d)))


def test_a_rotation_by_whole_sectors_rolls_the_descriptor_and_is_the_shift():
    E2, b = cs.default_tables()
    R, S = 20, 60
    rng = np.random.default_rng(7)
    heights = np.where(rng.random((R, S)) < 0.4, rng.integers(1, 40, (R, S)) * 0.25, 0.0).astype(F)
    cloud = scm.cell_centre_cloud(E2, b, heights)
    D = scm.descriptor(cloud, E2, b)
    assert np.array_equal(D, heights)
    for k in (1, 7, 30, 59):
        Dk = scm.descriptor(scm.rotate_z(cloud, k * 2.0 * np.pi / S), E2, b)
        assert np.array_equal(Dk, np.roll(D, k, axis=1)), k
        dist, shift = scm.distance(D, Dk)  # column j of the query lies on column j + k of the candidate
        assert shift == k and abs(dist) <= 1e-12, (k, dist, shift)
        assert np.allclose(scm.guess(k, S)[:3, :3] @ cloud[0], scm.rotate_z(cloud[:1], k * 2.0 * np.pi / S)[0], atol=1e-4)


def test_a_descriptor_matches_itself_at_shift_0():
    E2, b = cs.default_tables()
    Q = scm.descriptor(cs.drive_scans(12)[4], E2, b)
    dist, shift = scm.distance(Q, Q)
    assert shift == 0 and abs(dist) <= 1e-12


def test_equal_columns_tie_at_every_shift_and_report_shift_0():
    col = np.arange(1, 21, dtype=F) * F(0.25)
    Q = np.repeat(col[:, None], 60, axis=1)
    d = scm.shift_distances(Q, Q)
    assert (d == d[0]).all()
    assert scm.distance(Q, Q)[1] == 0


def test_an_empty_descriptor_is_at_distance_1():
    E2, b = cs.default_tables()
    Z = np.zeros((20, 60), dtype=F)
    Q = scm.descriptor(cs.drive_scans(12)[0], E2, b)
    assert scm.distance(Z, Q) == (1.0, 0) and scm.distance(Q, Z) == (1.0, 0) and scm.distance(Z, Z) == (1.0, 0)
    assert np.array_equal(scm.descriptor(np.zeros((0, 3), dtype=F), E2, b), Z)


def test_ranking_is_by_distance_then_id():
    assert scm.ranking([0.5, 0.25, 0.5, 0.125], first=10).tolist() == [13, 11, 10, 12]


def test_the_gpu_fixtures_keep_their_margins_and_find_the_place():
    """12 places, three yawed and moved revisits: the right place is top-1, its shift is the yaw's sector or a neighbour, and no two
    values the GPU test must tell apart are closer than MARGIN"""
    E2, b = cs.default_tables()
    db = [scm.descriptor(s, E2, b) for s in cs.drive_scans(12)]
    for i in (3, 7, 10):
        scan, _ = cs.revisit(i, 12)
        Q = scm.descriptor(scan, E2, b)
        shift_gap, rank_gap = cs.margins(Q, db)
        assert shift_gap > cs.MARGIN and rank_gap > cs.MARGIN
        ids, dist, shift = scm.match(Q, db, 0, 12, 3)
        assert ids[0] == i
        assert abs(int(shift[0]) - round(cs.REVISIT_YAW_DEG / 6.0)) <= 1
