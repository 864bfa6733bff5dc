"""The rolling voxel map through the C++ shim (include/nano_gicp/nano_gicp.hpp: setVoxelRolling / getVoxelRolling / insertIntoVoxelMap /
evictVoxelMap / clearVoxelMap / rollingVoxelMap / voxelRollingStats), compiled with g++ -Wall -Werror (tests/cpp/vgicp_rolling_shim.cpp)
and, on the GPU, compared bit for bit with the Python API on the same clouds."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "vgicp_rolling_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vgicp_rolling_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_vgicp_rolling_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


def test_the_python_api_declares_the_rolling_entries():
    from direct_lidar_odometry_amd import nano_gicp
    names = ["ngicp_set_voxel_rolling", "ngicp_get_voxel_rolling", "ngicp_voxel_rolling_insert", "ngicp_voxel_rolling_evict",
             "ngicp_voxel_rolling_clear", "ngicp_voxel_rolling_get", "ngicp_voxel_rolling_stats"]
    assert all(n in nano_gicp.EXPORTS for n in names)
    header = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    assert all(f"int {n}(" in header for n in names)
    for m in ("setVoxelRolling", "getVoxelRolling", "insertIntoVoxelMap", "evictVoxelMap", "clearVoxelMap", "rollingVoxelMap", "voxelRollingStats"):
        assert callable(getattr(nano_gicp.NanoGICP, m))


@pytest.mark.gpu
def test_vgicp_rolling_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP
    sc = clouds.make_scene()
    scans = [clouds.vlp16(sc, clouds.make_pose((0.3 * i, 0.05 * i, 0.0), (0.0, 0.0, 1.0 * i)), 300 + i, cols=188) for i in range(3)]
    res = 1.0
    paths = []
    for i, a in enumerate(scans):
        p = tmp_path / f"scan{i}.bin"
        np.ascontiguousarray(a[:, :3], np.float32).tofile(p)
        paths.append(str(p))
    exe = _build(tmp_path)
    out = subprocess.run([exe, repr(res), *paths], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    rows = {l[0]: l[1:] for l in lines}  # (the last of a repeated tag)
    every = lambda tag: [l[1:] for l in lines if l[0] == tag]
    assert rows["rolling_default"] == ["0"] and rows["rolling"] == ["1"]

    def stats_row(g):
        s = g.voxelRollingStats()
        return [str(s["inserts"]), str(s["n_vox"]), str(s["capacity_vox"]), str(s["table_slots"])]

    g = NanoGICP()
    assert g.getVoxelRolling() is False
    g.setVoxelResolution(res)
    g.setVoxelRolling(True)
    assert g.getVoxelRolling() is True
    assert rows["stats_empty"][:4] == stats_row(g) == ["0", "0", "0", "0"]
    T = np.eye(4, dtype=np.float32)
    Ts, convs, inserts = every("T"), every("converged"), every("insert")
    for i, a in enumerate(scans):
        g.setInputSource(a)
        if i:
            g.align(T)
            T = g.getFinalTransformation().copy()
            T_cpp = np.array([float.fromhex(v) for v in Ts[i - 1]], np.float32).reshape(4, 4).T
            assert np.array_equal(T_cpp, T), f"scan {i}"
            assert [int(convs[i - 1][0]), int(convs[i - 1][2])] == [int(g.hasConverged()), g.nr_iterations_] and g.hasConverged()
        n_new, n_touched = g.insertIntoVoxelMap(g, T)
        assert inserts[i] == ["1", str(n_new), str(n_touched)]
    assert rows["stats_full"][:4] == stats_row(g) and int(rows["stats_full"][0]) == 3
    assert int(rows["voxels"][0]) == g.getVoxelMapSize() > 300
    assert int(rows["evicted"][0]) == g.evictVoxelMap(T[:3, 3], 10.0, 0) > 0
    ijk, s, c, cnt, st = g.rollingVoxelMap()
    assert [int(v) for v in rows["map"][:4]] == [len(ijk), int(cnt.sum()), int(st.sum()), int(ijk[0, 0])]
    assert float.fromhex(rows["map"][4]) == s[0, 0] and float.fromhex(rows["map"][5]) == c[0, 2, 2]
    assert rows["stats_evicted"][:4] == stats_row(g) and rows["stats_evicted"][4:] == ["1", "1"]
    g.clearVoxelMap()
    assert rows["stats_cleared"][:4] == stats_row(g) and rows["stats_cleared"][:2] == ["0", "0"]
    g.close()
