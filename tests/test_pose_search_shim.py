"""The voxel pose search on the host side: the public header, the Python API's export list and the C++ shim
(include/nano_gicp/nano_gicp.hpp: voxelPoseSearch / voxelPoseSearchScores / voxelPoseSearchKernelMs / yawLattice / poseSearchCandidate)
all declare it, the shim's use of it (tests/cpp/pose_search_shim.cpp) compiles with g++ -Wall -Werror, and the shim's candidate pose is
the numpy restatement of the definition, (float)((double)t + (double)s * res) per axis, bit for bit.  The program's run against the
Python API on a GPU is in tests/test_gpu_pose_search.py."""
import os
import subprocess

import numpy as np
import pytest

import _pose_search_model as psm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ["ngicp_voxel_pose_search", "ngicp_voxel_pose_search_scores", "ngicp_voxel_pose_search_kernel_ms"]
PY_METHODS = ["voxelPoseSearch", "voxelPoseSearchScores", "voxelPoseSearchKernelMs", "yawLattice", "poseSearchCandidate"]


def test_header_exports_and_shim_declare_the_pose_search_entries():
    from direct_lidar_odometry_amd import nano_gicp
    assert all(n in nano_gicp.EXPORTS for n in NAMES)
    header = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    assert all(f"int {n}(" in header for n in NAMES)
    assert "voxel pose search" in header and "ON CELLS" in header
    for m in PY_METHODS:
        assert callable(getattr(nano_gicp.NanoGICP, m)), m
    shim = open(os.path.join(ROOT, "include", "nano_gicp", "nano_gicp.hpp")).read()
    assert "struct PoseSearchCandidate {" in shim
    for m in PY_METHODS:
        assert f" {m}(" in shim, m


def test_the_python_helpers_are_the_model_s():
    from direct_lidar_odometry_amd import nano_gicp
    T0 = np.eye(4)
    T0[:3, 3] = (1.5, -2.0, 0.25)
    lat = nano_gicp.NanoGICP.yawLattice(T0, 72, np.radians(5.0))
    assert lat.dtype == F and lat.shape == (72, 4, 4)
    assert np.array_equal(lat, psm.yaw_lattice(T0, 72, np.radians(5.0)))
    assert np.array_equal(lat[0], T0.astype(F))
    rng = np.random.default_rng(11)
    for _ in range(200):
        T = lat[rng.integers(72)].copy()
        T[:3, 3] = rng.uniform(-100, 100, 3).astype(F)
        s = rng.integers(-31, 32, 3)
        res = float(rng.choice([0.1, 0.3, 0.5, 1.0, 1.0 / 3.0]))
        got = nano_gicp.NanoGICP.poseSearchCandidate(T, s, res)
        assert got.dtype == F and np.array_equal(got, psm.candidate_pose(T, s, res))


@pytest.fixture(scope="module")
def shim_exe(hip_lib, tmp_path_factory):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(tmp_path_factory.mktemp("pose_search_shim")), "pose_search_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_search_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_pose_search_shim_compiles(shim_exe):
    assert os.path.exists(shim_exe)


def test_the_shim_s_candidate_pose_is_the_definition(shim_exe):
    """the `candidate` mode touches no GPU: it only evaluates NanoGICP::poseSearchCandidate"""
    rng = np.random.default_rng(12)
    lat = psm.yaw_lattice(np.eye(4), 72, np.radians(5.0))
    for res in (0.1, 0.5, 1.0 / 3.0):
        for _ in range(8):
            T = lat[rng.integers(72)].copy()
            T[:3, 3] = rng.uniform(-100, 100, 3).astype(F)
            s = [int(v) for v in rng.integers(-31, 32, 3)]
            args = [shim_exe, "candidate", float(res).hex(), *map(str, s), *[float(v).hex() for v in T.T.reshape(-1)]]
            run = subprocess.run(args, capture_output=True, text=True, timeout=60)
            assert run.returncode == 0, run.stdout + run.stderr
            tok = run.stdout.split()
            assert tok[0] == "candidate"
            got = np.array([float.fromhex(t) for t in tok[1:]], dtype=F).reshape(4, 4).T
            assert np.array_equal(got, psm.candidate_pose(T, s, res)), (res, s)
