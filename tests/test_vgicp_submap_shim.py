"""The merged voxel map through the C++ shim (include/nano_gicp/nano_gicp.hpp: setVoxelSubmapMerge / getVoxelSubmapMerge /
voxelMapMergeStats / keyframeVoxelMap), compiled with g++ -Wall -Werror (tests/cpp/vgicp_submap_shim.cpp) and, on the GPU, compared bit
for bit with the Python API on the same clouds."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "vgicp_submap_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vgicp_submap_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_vgicp_submap_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_vgicp_submap_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP
    w = clouds.scan_to_submap(3008, 2)
    res = 1.0
    half = len(w.target) // 2
    kfs = [np.ascontiguousarray(w.target[:half, :3], np.float32), np.ascontiguousarray(w.target[half:, :3], np.float32)]
    paths = []
    for name, a in (("src", np.ascontiguousarray(w.source[:, :3], np.float32)), ("kf0", kfs[0]), ("kf1", kfs[1])):
        p = tmp_path / f"{name}.bin"
        a.tofile(p)
        paths.append(str(p))
    exe = _build(tmp_path)
    out = subprocess.run([exe, repr(res), *paths], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}
    assert rows["merge_default"] == ["0"] and rows["merge"] == ["1"]

    prod, g = NanoGICP(), NanoGICP()
    assert g.getVoxelSubmapMerge() is False
    g.setVoxelResolution(res)
    g.setVoxelSubmapMerge(True)
    assert g.getVoxelSubmapMerge() is True
    for a in kfs:
        prod.setInputSource(a)
        g.addKeyframeTransformed(prod, np.eye(4))
    g.setSubmapKeyframes([0, 1])
    st = g.voxelMapMergeStats()
    assert rows["stats_before"][:2] == [str(st["merged_builds"]), str(st["parts_built"])] == ["0", "0"]
    assert int(rows["voxels"][0]) == g.getVoxelMapSize() > 1000
    st = g.voxelMapMergeStats()
    assert rows["stats_merged"] == [str(st["merged_builds"]), str(st["parts_built"]), "1", "1"] == ["1", "2", "1", "1"]
    ijk, s, _, cnt = g.keyframeVoxelMap(1)
    assert [int(rows["part"][0]), int(rows["part"][1])] == [len(ijk), int(cnt.sum())] == [len(ijk), len(kfs[1])]
    assert float.fromhex(rows["part"][2]) == s[0, 0]
    g.setInputSource(w.source)
    g.align()
    T_cpp = np.array([float.fromhex(v) for v in rows["T"]], np.float32).reshape(4, 4).T
    assert np.array_equal(T_cpp, g.getFinalTransformation())
    assert [int(rows["converged"][0]), int(rows["converged"][2])] == [int(g.hasConverged()), g.nr_iterations_]
    g.setVoxelSubmapMerge(False)
    assert int(rows["voxels_off"][0]) == g.getVoxelMapSize() == int(rows["voxels"][0])
    st = g.voxelMapMergeStats()
    assert rows["stats_off"][:2] == [str(st["merged_builds"]), str(st["parts_built"])] == ["1", "2"]
    g.align()
    T_off = np.array([float.fromhex(v) for v in rows["T_off"]], np.float32).reshape(4, 4).T
    assert np.array_equal(T_off, g.getFinalTransformation())
    prod.close(); g.close()
