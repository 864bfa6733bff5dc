"""The voxel fitness entries on the host side: the public header, the Python API's export list and the C++ shim
(include/nano_gicp/nano_gicp.hpp: VoxelFitness / getVoxelFitness / getVoxelFitnessScores / voxelFitnessPoints) all declare them, and the
shim's use of them (tests/cpp/voxel_fitness_shim.cpp) compiles with g++ -Wall -Werror.  The program's run against the Python API is in
tests/test_gpu_voxel_fitness.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ngicp_voxel_fitness", "ngicp_voxel_fitness_batch", "ngicp_voxel_fitness_points"]
PY_METHODS = ["voxelFitness", "voxelFitnessBatch", "voxel_fitness_points"]
SHIM_METHODS = ["getVoxelFitness", "getVoxelFitnessScores", "voxelFitnessPoints"]


def test_header_exports_and_shim_declare_the_voxel_fitness_entries():
    from direct_lidar_odometry_amd import nano_gicp
    assert all(n in nano_gicp.EXPORTS for n in NAMES)
    header = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    assert all(f"int {n}(" in header for n in NAMES)
    assert "ngicp_voxel_fitness_t;" in header and "voxel fitness" in header
    for m in PY_METHODS:
        assert callable(getattr(nano_gicp.NanoGICP, m)), m
    shim = open(os.path.join(ROOT, "include", "nano_gicp", "nano_gicp.hpp")).read()
    assert "struct VoxelFitness {" in shim
    for m in SHIM_METHODS:
        assert f" {m}(" in shim, m
    # the exact score's entries are as they were
    assert "double getFitnessScore(double max_range" in shim and "std::vector<double> getFitnessScores(" in shim


def test_the_record_has_the_header_s_layout():
    import ctypes as C
    from direct_lidar_odometry_amd import nano_gicp
    assert [f[0] for f in nano_gicp.VoxelFitness._fields_] == ["mahalanobis", "sqdist", "n_inliers", "n_matched"]
    assert C.sizeof(nano_gicp.VoxelFitness) == 2 * 8 + 2 * C.sizeof(C.c_size_t) == nano_gicp.NanoGICP._VFIT_DTYPE.itemsize


def test_voxel_fitness_shim_compiles(hip_lib, tmp_path):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(tmp_path), "voxel_fitness_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "voxel_fitness_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert os.path.exists(exe)
