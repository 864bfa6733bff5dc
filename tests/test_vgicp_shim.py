"""Voxelized GICP through the C++ shim (include/nano_gicp/nano_gicp.hpp: setVoxelResolution / getVoxelResolution / getVoxelMapSize),
compiled with g++ -Wall -Werror (tests/cpp/vgicp_shim.cpp) and, on the GPU, compared bit for bit with the Python API on the same clouds."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "vgicp_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vgicp_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_vgicp_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_vgicp_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP
    w = clouds.scan_to_submap(3008, 2)
    res = 1.0
    paths = []
    for name, a in (("src", w.source), ("tgt", w.target)):
        p = tmp_path / f"{name}.bin"
        np.ascontiguousarray(a[:, :3], np.float32).tofile(p)
        paths.append(str(p))
    exe = _build(tmp_path)
    out = subprocess.run([exe, *paths, repr(res)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}
    assert float.fromhex(rows["resolution_default"][0]) == 0.0 and float.fromhex(rows["resolution"][0]) == res

    g = NanoGICP()
    assert g.getVoxelResolution() == 0.0
    g.setVoxelResolution(res)
    g.setInputSource(w.source); g.setInputTarget(w.target)
    assert int(rows["voxels"][0]) == g.getVoxelMapSize() > 1000
    g.align()
    T_cpp = np.array([float.fromhex(v) for v in rows["T"]], np.float32).reshape(4, 4).T
    assert np.array_equal(T_cpp, g.getFinalTransformation())
    assert [int(rows["converged"][0]), int(rows["converged"][2])] == [int(g.hasConverged()), g.nr_iterations_]
    g.setVoxelResolution(0.0)
    g.align()
    T_exact = np.array([float.fromhex(v) for v in rows["T_exact"]], np.float32).reshape(4, 4).T
    assert np.array_equal(T_exact, g.getFinalTransformation()) and not np.array_equal(T_exact, T_cpp)
