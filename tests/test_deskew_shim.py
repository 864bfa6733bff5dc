"""The motion deskew through the C++ shim (include/nano_gicp/nano_gicp.hpp: DeskewTrajectory, deskewCloud, preprocessScanDeskewed),
compiled with g++ -Wall -Werror (tests/cpp/deskew_shim.cpp) and, on the GPU, compared bit for bit with the Python API."""
import os
import subprocess

import numpy as np
import pytest

import _deskew_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "deskew_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "deskew_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_deskew_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


def _rows(lines, tag):
    return np.array([[float.fromhex(v) for v in l[1:]] for l in lines if l[0] == tag], np.float64).astype(np.float32)


@pytest.mark.gpu
def test_deskew_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP
    scan = clouds.vlp16(clouds.make_scene(), clouds.make_pose(), noise_seed=3, cols=63)  # 1008 points
    tau, poses = dc.twist_trajectory((5.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.1, 11)
    times = clouds.sweep_times(len(scan)).astype(np.float32)
    times[17] = np.nan  # dropped by removeNaN in the preprocess route, NaN in the host-to-host route
    raw = clouds.skew_scan(scan, np.nan_to_num(times.astype(np.float64)), tau, poses, poses[-1])
    paths = [str(tmp_path / name) for name in ("scan.bin", "times.bin", "traj.bin")]
    raw.tofile(paths[0])
    times.tofile(paths[1])
    np.c_[tau, poses.transpose(0, 2, 1).reshape(len(tau), 16)].astype(np.float64).tofile(paths[2])
    res = subprocess.run([_build(tmp_path), *paths], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = [l.split() for l in res.stdout.splitlines()]

    g = NanoGICP()
    want = g.deskewCloud(raw, times, tau, poses, poses[-1])
    got = _rows(lines, "cloud")
    assert np.array_equal(got[:, :3].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, 3], np.arange(len(scan), dtype=np.float32))  # the other fields of the records are kept
    pre = _rows(lines, "scan")
    keep = np.arange(len(scan)) != 17
    assert np.array_equal(pre[:, :3].view(np.uint32), want[keep].view(np.uint32)) and np.array_equal(pre[:, 3], np.arange(len(scan), dtype=np.float32)[keep])
    g.setInputSource(want[keep])
    median = [l for l in lines if l[0] == "median"]
    assert np.float32(float.fromhex(median[0][1])).tobytes() == g.medianRange().tobytes()  # the deskewed scan became the source
    assert [l for l in lines if l[0] == "refused"] == [["refused", "1", "1", str(len(scan))]]
    g.close()
