"""The voxelized-GICP neighbourhoods through the C++ shim (include/nano_gicp/nano_gicp.hpp: NeighborSearchMethod,
setNeighborSearchMethod / getNeighborSearchMethod / voxelCorrespondences), compiled with g++ -Wall -Werror
(tests/cpp/vgicp_nbr_shim.cpp) and, on the GPU, compared bit for bit with the Python API on the same clouds."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "vgicp_nbr_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vgicp_nbr_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_vgicp_nbr_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_vgicp_nbr_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP, NeighborSearchMethod
    w = clouds.scan_to_submap(3008, 2)
    res = 1.0
    paths = []
    for name, a in (("src", w.source), ("tgt", w.target)):
        p = tmp_path / f"{name}.bin"
        np.ascontiguousarray(a[:, :3], np.float32).tofile(p)
        paths.append(str(p))
    corr_path = str(tmp_path / "corr.bin")
    exe = _build(tmp_path)
    out = subprocess.run([exe, *paths, repr(res), corr_path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}
    assert int(rows["neighbors_default"][0]) == 1 and int(rows["neighbors"][0]) == 7

    g = NanoGICP()
    assert g.getNeighborSearchMethod() == NeighborSearchMethod.DIRECT1
    g.setVoxelResolution(res)
    g.setNeighborSearchMethod(NeighborSearchMethod.DIRECT7)
    g.setInputSource(w.source); g.setInputTarget(w.target)
    g.align()
    T_cpp = np.array([float.fromhex(v) for v in rows["T"]], np.float32).reshape(4, 4).T
    assert np.array_equal(T_cpp, g.getFinalTransformation())
    assert [int(rows["converged"][0]), int(rows["converged"][2])] == [int(g.hasConverged()), g.nr_iterations_]
    corr = g.voxel_correspondences()
    assert corr.shape == (len(w.source), 7) and int(rows["corr_ints"][0]) == corr.size
    corr_cpp = np.fromfile(corr_path, np.int32).reshape(-1, 7)
    assert np.array_equal(corr_cpp, corr) and ((corr >= 0).sum(axis=1) > 1).any()
    g.setNeighborSearchMethod(NeighborSearchMethod.DIRECT27)
    g.align()
    T27 = np.array([float.fromhex(v) for v in rows["T27"]], np.float32).reshape(4, 4).T
    assert np.array_equal(T27, g.getFinalTransformation()) and not np.array_equal(T27, T_cpp)
    assert int(rows["corr27_ints"][0]) == len(w.source) * 27
    g.close()
