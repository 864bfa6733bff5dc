"""Clearing the rolling map along rays through the C++ shim (include/nano_gicp/nano_gicp.hpp: clearVoxelMapAlongRays / voxelMapRayCounts),
compiled with g++ -Wall -Werror (tests/cpp/vgicp_ray_shim.cpp) and, on the GPU, compared byte for byte with the Python API on the same
clouds: the counts, the totals, the surviving map, and a refusal."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ngicp_voxel_rolling_ray_clear", "ngicp_voxel_rolling_ray_counts"]


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "vgicp_ray_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vgicp_ray_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_vgicp_ray_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


def test_header_python_and_shim_declare_the_ray_entries(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    assert all(n in nano_gicp.EXPORTS for n in NAMES) and all(hasattr(hip_lib, n) for n in NAMES)
    header = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    assert all(f"int {n}(" in header for n in NAMES)
    assert "typedef struct ngicp_ray_clear_options" in header and "typedef struct ngicp_ray_clear_result" in header
    shim = open(os.path.join(ROOT, "include", "nano_gicp", "nano_gicp.hpp")).read()
    assert all(f"{n}(h_" in shim for n in NAMES)
    for m in ("clearVoxelMapAlongRays", "voxelMapRayCounts"):
        assert callable(getattr(nano_gicp.NanoGICP, m)) and m in shim
    # the Python mirror of the options has the header's fields, in its order, with its defaults
    fields = [f for f, _ in nano_gicp.RayClearOptions._fields_]
    assert fields == ["near_cells", "back_cells", "max_steps", "min_miss", "radius_cells", "keep_stamp", "dry_run"]
    at = [header.index(f" {f};") for f in fields]
    assert at == sorted(at)
    assert nano_gicp.RayClearOptions.DEFAULTS == dict(near_cells=1, back_cells=2, max_steps=4096, min_miss=2, radius_cells=0.25, keep_stamp=0, dry_run=0)


@pytest.mark.gpu
def test_vgicp_ray_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP, NgicpError
    sc = clouds.make_scene()
    t = (0.75, -0.5, 0.125)  # (exact in float: the shim parses them from text)
    scans = [clouds.vlp16(sc, clouds.make_pose(p, (0.0, 0.0, 0.0)), 400 + i, cols=100) for i, p in enumerate(((0.0, 0.0, 0.0), t))]
    res = 1.0
    paths = []
    for i, a in enumerate(scans):
        p = tmp_path / f"scan{i}.bin"
        np.ascontiguousarray(a[:, :3], np.float32).tofile(p)
        paths.append(str(p))
    exe = _build(tmp_path)
    out = subprocess.run([exe, repr(res), *[repr(v) for v in t], *paths], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    rows = {l[0]: l[1:] for l in lines}  # (the last of a repeated tag)
    ints = lambda tag, dt=np.int64: np.array([int(v) for v in rows[tag]], dt)
    hexes = lambda tag: np.array([float.fromhex(v) for v in rows[tag]])

    def same_map(tag, g):
        ijk, s, c, cnt, st = g.rollingVoxelMap()
        assert [int(v) for v in rows[tag + "_n"]] == [len(ijk), g.voxelRollingStats()["inserts"]]
        assert np.array_equal(ints(tag + "_ijk"), ijk.reshape(-1)) and np.array_equal(ints(tag + "_count"), cnt) and np.array_equal(ints(tag + "_stamp"), st)
        assert hexes(tag + "_sum").tobytes() == s.tobytes()
        assert hexes(tag + "_covsum").tobytes() == np.ascontiguousarray(c.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]]).tobytes()

    def same_counts(tag, g):
        miss, hit = g.voxelMapRayCounts()
        assert rows[tag + "_ok"] == ["1", str(len(miss))]
        assert np.array_equal(ints(tag + "_miss", np.uint32), miss) and np.array_equal(ints(tag + "_hit", np.uint32), hit)

    def result_row(r):
        return ["1", str(r["n_removed"]), str(r["steps"]), str(r["occupied"]), str(r["misses"]), "1"]

    inserts = [l[1:] for l in lines if l[0] == "insert"]
    g = NanoGICP()
    g.setVoxelResolution(res); g.setVoxelRolling(True)
    assert rows["before_ok"] == ["0", "0"]
    with pytest.raises(NgicpError):
        g.voxelMapRayCounts()
    T = np.eye(4, dtype=np.float32)
    g.setInputSource(scans[0])
    assert inserts[0] == ["1", *map(str, g.insertIntoVoxelMap(g, T))]
    g.setInputSource(scans[1])
    T[:3, 3] = t
    dry = g.clearVoxelMapAlongRays(g, T, dry_run=1)
    assert rows["dry"] == result_row(dry) and dry["n_removed"] == 0 and dry["misses"] > 0
    same_counts("dry", g)
    with pytest.raises(NgicpError) as e:
        g.clearVoxelMapAlongRays(g, T, near_cells=0)
    assert e.value.code == -2 and rows["refused"] == ["0", "0", "0", "0", "0", "1"]
    same_counts("refused", g)  # the refusal left the dry run's counts readable, on both sides
    assert rows["refused_miss"] == rows["dry_miss"] and rows["refused_hit"] == rows["dry_hit"]
    same_map("kept", g)
    real = g.clearVoxelMapAlongRays(g, T, (t[0], t[1], t[2] + 0.25), radius_cells=0.5, min_miss=1)
    assert rows["clear"] == result_row(real) and real["n_removed"] > 0
    same_counts("clear", g)
    same_map("cleared", g)
    assert int(rows["cleared_n"][0]) == int(rows["kept_n"][0]) - real["n_removed"]
    assert inserts[1] == ["1", *map(str, g.insertIntoVoxelMap(g, T))]
    assert rows["stale_ok"] == ["0", "0"]
    with pytest.raises(NgicpError):
        g.voxelMapRayCounts()
    g.close()
