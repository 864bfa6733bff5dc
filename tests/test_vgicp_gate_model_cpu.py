"""The numpy model of the gated insert (tests/_vgicp_gate_model.py) proves itself on the CPU: the fixture puts points into every class and
keeps every term away from the gates, the identities of include/ngicp.h ("rolling voxel map: gated insert") hold on the model, and the
drive's parameters and figures - which the GPU test and DESIGN.md 4.24 take from here, not from the engine - are pinned."""
import numpy as np
import pytest

import _vgicp_gate_model as gm
import _vgicp_rolling_model as rm
import _voxel_fitness_model as fm

BIG = [n for n in gm.SIZES if n >= 255]


@pytest.fixture(scope="module")
def fixture_map():
    return gm.build_map()


def test_fixture_map_has_voxels_of_every_weight(fixture_map):
    c = fixture_map.count
    print(f"{len(c)} voxels: {int((c == 1).sum())} of one point, {int((c == 2).sum())} of two, {int((c >= gm.FIX_MIN_COUNT).sum())} of {gm.FIX_MIN_COUNT} or more, largest {c.max()}")
    assert (c == 1).sum() >= 20 and (c == 2).sum() >= 20 and (c >= 6).sum() >= 100 and fixture_map.inserts == 3


@pytest.mark.parametrize("n", BIG)
def test_every_class_holds_a_twentieth_of_the_source(fixture_map, n):
    src, cv = gm.source(n)
    cls, _, _ = gm.classify(src, cv, fixture_map, gm.SRC_POSE, 7, gm.FIX_GATE, gm.FIX_MIN_COUNT)
    share = np.bincount(cls, minlength=4) / n
    print(f"n = {n}: NEW {share[0]:.3f}, EXPLAINED {share[1]:.3f}, CONFLICT {share[2]:.3f}, UNJUDGED {share[3]:.3f}")
    assert (share >= gm.FLOOR).all()


@pytest.mark.parametrize("K", gm.NEIGHBORS)
@pytest.mark.parametrize("min_count", [1, gm.FIX_MIN_COUNT])
def test_no_term_sits_on_a_gate_or_on_its_runner_up(fixture_map, K, min_count):
    worst_gate, worst_gap = np.inf, np.inf
    for n in gm.SIZES:
        src, cv = gm.source(n)
        _, best, slot_m = gm.classify(src, cv, fixture_map, gm.SRC_POSE, K, gm.FIX_GATE, min_count)
        worst_gate = min(worst_gate, fm.gate_margin(best[np.isfinite(best)], gm.GATES))
        worst_gap = min(worst_gap, fm.slot_gap(slot_m))
    print(f"K = {K}, min_voxel_count = {min_count}: closest gate {worst_gate:.2e} relative, closest runner-up {worst_gap:.2e} relative")
    assert worst_gate >= gm.MARGIN and worst_gap >= gm.MARGIN


@pytest.mark.parametrize("K", gm.NEIGHBORS)
def test_no_gate_is_the_plain_insert(K):
    src, cv = gm.source(700)
    a, b = gm.build_map(), gm.build_map()
    out = gm.gated_insert(a, src, cv, gm.SRC_POSE, K, gm.DBL_MAX)
    assert (out["n_new"], out["n_touched"]) == b.insert(src, cv, gm.SRC_POSE)
    assert a.snapshot() == b.snapshot() and out["n_kept"] == 700 and out["n_class"][gm.CONFLICT] == 0
    # ... on an empty map too, where every point is NEW
    a, b = rm.RollingVoxelMap(gm.RES), rm.RollingVoxelMap(gm.RES)
    out = gm.gated_insert(a, src, cv, gm.SRC_POSE, K, 0.0)
    b.insert(src, cv, gm.SRC_POSE)
    assert a.snapshot() == b.snapshot() and out["n_class"] == [700, 0, 0, 0] and (out["cls"] == gm.NEW).all()


@pytest.mark.parametrize("K", gm.NEIGHBORS)
def test_run_of_gated_inserts_keeps_its_terms_off_the_gates(K):
    """the states of gm.RUN (the GPU test drives the engine through them): margins as above on every one, and the counter's steps"""
    m = rm.RollingVoxelMap(gm.RES)
    kept = []
    for i, (n, T, max_m, opt) in enumerate(gm.RUN):
        src, cv = gm.source(n, seed=900 + i)
        _, best, slot_m = gm.classify(src, cv, m, T, K, max_m, opt.get("min_voxel_count", 1))
        assert fm.gate_margin(best[np.isfinite(best)], [max_m]) >= gm.MARGIN and fm.slot_gap(slot_m) >= gm.MARGIN, (K, i)
        out = gm.gated_insert(m, src, cv, T, K, max_m, **opt)
        kept.append(out["n_kept"])
        print(f"DIRECT{K}, call {i}: {out['n_class']}, kept {out['n_kept']}, {len(m)} voxels, counter {m.inserts}")
    assert kept[2] == 0 and all(k > 0 for k in kept[:2] + kept[3:]) and m.inserts == len(gm.RUN) - 1 and len(set(m.stamp.tolist())) > 1


def test_nothing_kept_leaves_map_and_counter():
    src, cv = gm.source(257)
    empty = rm.RollingVoxelMap(gm.RES)
    before = empty.snapshot()
    out = gm.gated_insert(empty, src, cv, gm.SRC_POSE, 7, 2.5, insert_new=0)
    assert out["n_kept"] == 0 and out["n_class"] == [257, 0, 0, 0] and empty.snapshot() == before and empty.inserts == 0 and len(empty) == 0
    m = gm.build_map()
    before = m.snapshot()
    out = gm.gated_insert(m, src, cv, gm.SRC_POSE, 7, 0.0, insert_new=0, insert_unjudged=0)  # (a gate of 0: every judged point is a CONFLICT)
    assert out["n_kept"] == 0 and out["n_class"][gm.EXPLAINED] == 0 and out["n_class"][gm.CONFLICT] > 0
    assert m.snapshot() == before and m.inserts == 3
    out = gm.gated_insert(m, src, cv, gm.SRC_POSE, 7, 2.5, dry_run=1)
    assert out["n_kept"] > 0 and (out["n_new"], out["n_touched"]) == (0, 0) and m.snapshot() == before


def test_refusal_is_judged_on_every_point(fixture_map):
    src, cv = gm.source(65)
    far = src.copy()
    far[3] = (0.0, 0.0, 0.3 + 2.0 ** 20 * gm.RES)  # (its gate point has no cell, so it is NEW - and dropped with insert_new = 0 - yet it refuses)
    before = fixture_map.snapshot()
    for bad in (far, np.r_[src[:10], [[np.nan, 0, 0]], src[10:]].astype(np.float32)):
        with pytest.raises(rm.Refused):
            gm.gated_insert(fixture_map, bad, gm.covs(len(bad), 1), fm.pose(), 7, 2.5, insert_new=0)
    assert fixture_map.snapshot() == before


@pytest.mark.parametrize("K", gm.NEIGHBORS)
def test_classes_follow_from_point_values(fixture_map, K):
    src, cv = gm.source(700)
    m, _, v, matched, _ = fm.point_values(src, cv, fixture_map, gm.SRC_POSE, K)
    for gate in gm.GATES:
        cls, _, _ = gm.classify(src, cv, fixture_map, gm.SRC_POSE, K, gate, 1)
        assert np.array_equal(cls, gm.classes_from_point_values(m, v, gate)), (K, gate)
        assert np.array_equal(cls == gm.NEW, ~matched)
    assert (gm.classify(src, cv, fixture_map, gm.SRC_POSE, K, 2.5, 1)[0] != gm.UNJUDGED).all()  # (every voxel of this map gives a finite term)


def test_drive_parameters_and_figures():
    """the room with the moving box (tests/_vgicp_ray_drive.py), every second ray, inserted at the true pose: what the gate is for.
    These figures are the model's; DESIGN.md 4.24 quotes them and the GPU test holds the engine to the same maps."""
    plain, gated, results = gm.drive_model(gm.DRIVE_GATE, gm.DRIVE_MIN_COUNT, gm.DRIVE_WARMUP)
    trail_plain, trail_gated, lost, static = gm.drive_figures(plain, gated)
    print(f"gate {gm.DRIVE_GATE}, min_voxel_count {gm.DRIVE_MIN_COUNT}, {gm.DRIVE_WARMUP} ungated frame(s), DIRECT{gm.DRIVE_K} at {gm.DRIVE_RES} m: "
          f"{trail_plain} trail voxels without the gate, {trail_gated} with it; {lost} of {static} static voxels lost (cap {gm.DRIVE_LOST_CAP})")
    for f, r in enumerate(results, start=gm.DRIVE_WARMUP):
        print(f"  frame {f}: NEW {r['n_class'][0]}, EXPLAINED {r['n_class'][1]}, CONFLICT {r['n_class'][2]}, UNJUDGED {r['n_class'][3]}")
    assert (trail_plain, trail_gated, lost, static) == gm.DRIVE_FIGURES
    for r in results:  # (no term of the drive sits on its gate either)
        assert fm.gate_margin(r["best"][np.isfinite(r["best"])], [gm.DRIVE_GATE]) >= gm.MARGIN and fm.slot_gap(r["slot_m"]) >= gm.MARGIN
    assert trail_gated < trail_plain and lost <= gm.DRIVE_LOST_CAP == static // 20
    # a chi-square-sized gate keeps the whole scan here: the plane-regularised covariances are 1 along a surface, so m sees only the offset across it
    _, loose, _ = gm.drive_model(7.8, 1, 1)
    assert gm.drive_figures(plain, loose)[1] >= trail_plain - 1
