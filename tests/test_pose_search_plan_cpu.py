"""The pose search's planning header (direct_lidar_odometry_amd/csrc/ngicp_pose_search_plan.h: caps, shift index, the occupancy grid's
plan) compiled into a stand-alone program with its own main (tests/cpp/pose_search_plan.cpp; g++ -std=c++17 -Wall -Werror against the
header alone - no library, no GPU) and held to the numpy model's boxes and plan (tests/_pose_search_model.py); once more under
AddressSanitizer and UBSan."""
import os
import subprocess

import numpy as np
import pytest

import _pose_search_model as psm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LIM = psm.VOXEL_LIMIT


def _cases():
    """(map cells, base poses, source, resolution, extent) -> boxes through the model; plus boxes given directly"""
    rng = np.random.default_rng(3)
    eye = np.eye(4, dtype=F)[None]
    room = np.unique(rng.integers(-40, 41, (500, 3)), axis=0)
    src = rng.uniform(-6.0, 6.0, (200, 3)).astype(F)
    far = src + F(500.0)
    out = []
    for e in [(0, 0, 0), (3, 2, 1), (31, 31, 1), (12, 12, 1)]:
        out.append((psm.box_of(room), psm.source_box(psm.yaw_lattice(np.eye(4), 5, 0.9), src, 0.5), e))
        out.append((psm.box_of(room), psm.source_box(eye, far, 0.5), e))                    # empty intersection: the source is elsewhere
        out.append((psm.box_of([[7, -3, 2]]), psm.source_box(eye, src, 0.5), e))            # a one-cell map
        out.append((psm.box_of([[7, -3, 2]]), psm.box_of([[7 + e[0] + 1, -3, 2]]), e))      # ... one cell beyond the window: empty
        out.append((psm.box_of([[7, -3, 2]]), psm.box_of([[7 + e[0], -3 - e[1], 2 + e[2]]]), e))  # ... on the window's corner: one cell
        out.append((psm.box_of(room), psm.source_box(eye, np.full((3, 3), np.nan, dtype=F), 0.5), e))  # no point has a cell
        out.append((psm.EMPTY_BOX, psm.source_box(eye, src, 0.5), e))
    # boxes touching +-(2^20 - 1) on every axis
    out.append(((np.array([-(LIM - 1)] * 3), np.array([-(LIM - 1) + 2] * 3)), (np.array([-(LIM - 1)] * 3), np.array([-(LIM - 1)] * 3)), (31, 31, 1)))
    out.append(((np.array([LIM - 3] * 3), np.array([LIM - 1] * 3)), (np.array([LIM - 1] * 3), np.array([LIM - 1] * 3)), (31, 5, 7)))
    out.append(((np.array([-(LIM - 1), 0, 0]), np.array([LIM - 1, 3, 3])), (np.array([-(LIM - 1), 0, 0]), np.array([LIM - 1, 0, 0])), (1, 1, 1)))
    # the byte cap: 2^21 - 1 cells wide is 32770 words a row; 1024 rows are 256 MiB and 80 bytes a row over, 1023 are under
    wide = np.array([-(LIM - 1), 0, 0]), np.array([LIM - 1, 1023, 0])
    out.append((wide, wide, (0, 0, 0)))
    out.append(((wide[0], np.array([LIM - 1, 1022, 0])), wide, (0, 0, 0)))
    out.append(((np.array([-(LIM - 1)] * 3), np.array([LIM - 1] * 3)), (np.array([-(LIM - 1)] * 3), np.array([LIM - 1] * 3)), (31, 31, 1)))  # 2^57-ish bytes: no overflow
    return out


def _expected(case):
    p = psm.plan(*case)
    if p is None:
        return "empty"
    return "plan " + " ".join(str(int(v)) for v in [*p["org"], *p["n"], p["row_words"], p["bytes"], int(p["too_large"])])


@pytest.mark.parametrize("name,extra", [("pose_search_plan", []), ("pose_search_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_the_planning_header_matches_the_model(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "cpp", "pose_search_plan.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    cases = _cases()
    path = os.path.join(str(tmp_path), "cases.txt")
    with open(path, "w") as f:
        for mb, sb, e in cases:
            f.write(" ".join(str(int(v)) for v in [*mb[0], *mb[1], *sb[0], *sb[1], *e]) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases) + 1
    want = [_expected(c) for c in cases]
    assert lines[:-1] == want
    assert "empty" in want and any(w.endswith(" 1") for w in want) and any(w.endswith(" 0") for w in want)  # every kind of answer occurred
    tail = lines[-1].split()
    assert tail[0] == "checks" and int(tail[1]) > 1_000_000 and tail[2:] == ["failures", "0"]


def test_the_model_s_plan_covers_exactly_the_cells_a_window_can_reach():
    """brute force on a small case: a cell is in the planned grid iff it is in the map's box and is c + s for some cell c of the source's
    box and some shift s"""
    mb = (np.array([-2, 0, 1]), np.array([6, 3, 2]))
    sb = (np.array([4, -5, 1]), np.array([9, -2, 1]))
    e = (1, 3, 0)
    p = psm.plan(mb, sb, e)
    reach = set()
    for x in range(sb[0][0] - e[0], sb[1][0] + e[0] + 1):
        for y in range(sb[0][1] - e[1], sb[1][1] + e[1] + 1):
            for z in range(sb[0][2] - e[2], sb[1][2] + e[2] + 1):
                if all(mb[0][a] <= v <= mb[1][a] for a, v in enumerate((x, y, z))):
                    reach.add((x, y, z))
    grid = {(x, y, z) for x in range(p["org"][0], p["org"][0] + p["n"][0]) for y in range(p["org"][1], p["org"][1] + p["n"][1])
            for z in range(p["org"][2], p["org"][2] + p["n"][2])}
    assert grid == reach and len(grid) == 4 * 2 * 1
