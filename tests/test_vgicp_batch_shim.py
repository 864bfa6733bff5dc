"""alignBatchVoxel through the C++ shim (include/nano_gicp/nano_gicp.hpp), compiled with g++ -Wall -Werror
(tests/cpp/vgicp_batch_shim.cpp); on the GPU the program compares every lane with alignPoseOnly(guess) on the same object by memcmp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "vgicp_batch_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vgicp_batch_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_vgicp_batch_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_vgicp_batch_shim_lanes_equal_the_single_aligns(hip_lib, tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    assert "lanes_equal 5" in out.stdout.splitlines()
    its = {int(line.split()[5]) for line in out.stdout.splitlines() if line.startswith("lane ")}
    assert len(its) > 1, its  # the lanes did not all stop together
