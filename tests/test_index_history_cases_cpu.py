"""The inputs of tests/test_gpu_index_history.py do what its tests claim (no GPU): tests/_index_history_cases.py's numpy restatement
of the engine's grid says that the crowded clouds put more than 65 535 target points into one cell and in front of a batch box
inside a region row, that the recycled pair shares its grid, and that the memo chain hits, recovers and wraps as designed."""
import numpy as np
import pytest

import _index_history_cases as ic
from direct_lidar_odometry_amd import clouds


def _distinct(pts):
    return len(np.unique(np.ascontiguousarray(pts).view([("", pts.dtype)] * pts.shape[1]))) == len(pts)


@pytest.fixture(scope="module")
def row():
    src, tgt = ic.crowded_row()
    dims, h = ic.grid_of(tgt, ic.CROWDED["crowded_row"][0])
    return src, tgt, dims, h, ic.cell_counts(tgt, tgt.min(0), h, dims)


# ------------------------------------------------------------------ A
def test_crowded_cell_is_one_cell_past_the_field():
    src, tgt = ic.crowded_cell()
    voxel, want, _ = ic.CROWDED["crowded_cell"]
    assert src.dtype == tgt.dtype == np.float32 and src.shape == (440, 3) and tgt.shape == (70_000, 3)
    dims, h = ic.grid_of(tgt, voxel)
    assert dims == want == [1, 1, 1] and h == np.float32(voxel)
    assert ic.cell_counts(tgt, tgt.min(0), h, dims) == {(0, 0, 0): 70_000} and 70_000 > ic.FIELD_MAX
    assert _distinct(tgt)
    assert ic.grid_of(src, voxel)[0] == [1, 1, 1]


def test_crowded_row_grid_and_populations(row):
    src, tgt, dims, h, counts = row
    assert src.dtype == tgt.dtype == np.float32 and src.shape == (640, 3) and tgt.shape == (175_000, 3)
    assert dims == ic.CROWDED["crowded_row"][1] == [5, 1, 1] and h == np.float32(1.0)
    assert np.array_equal(tgt.min(0), np.zeros(3, np.float32))  # the origin is exact: cell i is [i, i + 1)
    assert counts == {(i, 0, 0): 35_000 for i in range(5)}
    assert _distinct(tgt)


@pytest.mark.parametrize("moved", [False, True], ids=["as given", "under the guess"])
def test_crowded_row_saturates_both_fields(row, moved):
    """A batch in cell 3 or 4 has more than 65 535 target points in front of its box inside any region row that holds it, whatever
    the growth (2 .. 6); a batch in cell 0 has none and 35 000 up to its box's end (both fields as they are), one in cell 1 has
    35 000 and 70 000 (the second field saturated)."""
    src, tgt, dims, h, counts = row
    pts = clouds.transform_points(ic.CROWDED["crowded_row"][2], src) if moved else src
    inliers = pts[:600]
    own = ic.cell_coords(inliers, tgt.min(0), h, dims)
    inside = (np.floor(inliers) == np.c_[np.repeat(ic.ROW_SOURCE_CELLS, 120), np.zeros((600, 2))]).all(1)
    print(f"source points in their cell: {int(inside.sum())} of 600")
    occupied = sorted({tuple(int(v) for v in c) for c in own[inside]})
    assert occupied == [(i, 0, 0) for i in range(5)]
    assert dims[0] <= ic.STAGE_XS  # the whole row is a region row at any growth
    for grow in (2, 3, 4, 5, 6):
        front = {c[0]: ic.points_in_front(counts, c, grow) for c in occupied}
        upto = {c[0]: front[c[0]] + counts[c] for c in occupied}
        print(f"grow {grow}: points in front of a box in cell i {front}, up to its end {upto}")
        assert front[3] >= 65_536 and front[4] >= 65_536 and min(front[3], front[4]) > ic.FIELD_MAX
        assert front[0] == 0 and upto[0] == 35_000 <= ic.FIELD_MAX  # unsaturated
        assert front[1] == 35_000 <= ic.FIELD_MAX < upto[1] == 70_000  # half saturated
    # the staged route's table: the start of a row's third cell is already past the field (rw_b[][2], ngicp_pass_st.h)
    assert counts[(3, 0, 0)] + counts[(4, 0, 0)] > ic.FIELD_MAX


# ------------------------------------------------------------------ B
def test_recycle_pair_shares_its_grid():
    s1, s2, tgt = ic.recycle_pair()
    assert s1.shape == s2.shape == (3000, 3) and s1.dtype == s2.dtype == np.float32
    assert np.array_equal(s1.min(0), s2.min(0)) and np.array_equal(s1.max(0), s2.max(0))
    g1, g2 = ic.grid_of(s1, ic.RECYCLE_VOXEL), ic.grid_of(s2, ic.RECYCLE_VOXEL)
    assert g1 == g2 and g1[1] == np.float32(ic.RECYCLE_VOXEL) and min(g1[0]) > 4
    c1, c2 = (ic.cell_counts(s, s.min(0), g1[1], g1[0]) for s in (s1, s2))
    assert c1 != c2 and not np.array_equal(s1, s2)
    assert np.array_equal(s2[::-1, 1:], s1[:, 1:])


def test_tiny_clouds():
    small, one = ic.tiny_clouds()
    assert small.shape == (40, 3) and len(one) == 9
    for voxel in ic.TINY_VOXEL.values():
        assert ic.grid_of(one, voxel)[0] == [1, 1, 1]
        assert np.prod(ic.grid_of(small, voxel)[0]) >= 27


def test_capped_voxel_cloud():
    """The crowded row's target at voxel 0.02 would need 251 x 45 x 45 cells: inside the caps.  The recycled-object test takes the wide
    memo cloud at 0.02 instead, where make_grid has to grow the voxel."""
    wide = ic.memo_clouds()["wide"]
    dims, h = ic.grid_of(wide, 0.02)
    assert h > np.float32(0.02) and np.prod(dims) <= ic.MAX_CELLS and np.prod(dims) > ic.MAX_CELLS // 4, (dims, h)


# ------------------------------------------------------------------ C
@pytest.fixture(scope="module")
def memo():
    c = ic.memo_clouds()
    return c, ic.memo_walk(ic.MEMO_CHAIN, c), ic.memo_walk(ic.MEMO_REVERSE, c), {n: ic.fresh_voxel(c[n]) for n in ("dense", "wide")}


def test_memo_clouds(memo):
    c = memo[0]
    assert [len(c[k]) for k in ("dense", "wide", "n500", "n2000", "n40000", "n90000", "n150", "source")] == [12_000, 15_000, 500, 2000, 40_000, 90_000, 150, 3000]
    assert all(v.dtype == np.float32 for v in c.values())
    assert np.all(np.ptp(c["dense"], 0) < 3.0) and np.all(np.ptp(c["wide"], 0) > np.array([299.0, 299.0, 19.9]))


def test_first_memo_hit_is_real(memo):
    _, chain, rev, fresh = memo
    for w in (chain, rev):
        print([(n, round(h, 4), d, hit) for n, h, d, hit in w])
    print("fresh:", fresh)
    name, h, dims, hit = chain[1]
    assert name == "wide" and hit and not chain[0][3]
    assert fresh["wide"][0] / h > 4 and np.prod(dims) > 1 << 24  # the wide cloud under the dense cloud's voxel: a grid near the cap
    name, h, dims, hit = rev[1]
    assert name == "dense" and hit and not rev[0][3]
    assert h / fresh["dense"][0] > 4 and dims == [1, 1, 1]       # the dense cloud under the wide cloud's voxel: one cell


def test_memo_moves_back_step_by_step(memo):
    _, chain, rev, fresh = memo
    for w, name in ((chain[1:4], "wide"), (rev[1:4], "dense")):
        off = [abs(np.log(h / fresh[name][0])) for n, h, _, _ in w]
        assert all(n == name for n, _, _, _ in w) and off[0] > off[1] > off[2], off
        assert all(max(a / b, b / a) <= 4.0 + 1e-6 for a, b in zip([x[1] for x in w], [x[1] for x in w][1:]))


def test_memo_slots_wrap(memo):
    """n90000 finds no slot of its class and none empty: it takes the oldest (slot 0: the source's, which n2000 had taken over).  The
    12-15k class sits in slot 1 and survives that: the dense cloud after it is still a memo hit, at the voxel the wide clouds left.
    n150 then takes slot 1, and the dense cloud after THAT is indexed like the first one."""
    _, chain, _, fresh = memo
    by = {i: v for i, v in enumerate(chain)}
    assert [v[0] for v in chain] == list(ic.MEMO_CHAIN)
    assert [by[i][3] for i in (4, 6, 7, 9)] == [False] * 4 and by[5][3]  # n500, n40000, n90000, n150 are new classes; n2000 is the source's
    assert by[8][0] == "dense" and by[8][3] and by[8][1] / by[0][1] > 4
    assert by[10][0] == "dense" and not by[10][3] and by[10][1] == by[0][1] == fresh["dense"][0] and by[10][2] == by[0][2]
