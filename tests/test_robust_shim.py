"""The robust kernel through the C++ shim (include/nano_gicp/nano_gicp.hpp: RobustKernel, setRobustKernel / getRobustKernel /
robustTerms), compiled with g++ -Wall -Werror (tests/cpp/robust_shim.cpp) and, on the GPU, compared bit for bit with the Python API on
the same clouds: DIRECT7 with a Cauchy kernel."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "robust_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "robust_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_robust_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_robust_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP, NeighborSearchMethod, RobustKernel
    w = clouds.scan_to_submap(3008, 2)
    res, width = 1.0, 2.0
    paths = []
    for name, a in (("src", w.source), ("tgt", w.target)):
        p = tmp_path / f"{name}.bin"
        np.ascontiguousarray(a[:, :3], np.float32).tofile(p)
        paths.append(str(p))
    terms_path = str(tmp_path / "terms.bin")
    exe = _build(tmp_path)
    out = subprocess.run([exe, *paths, repr(res), repr(width), terms_path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}
    assert int(rows["kernel_default"][0]) == 0
    assert int(rows["kernel"][0]) == int(RobustKernel.CAUCHY) and float.fromhex(rows["kernel"][1]) == width

    g = NanoGICP()
    assert g.getRobustKernel()[0] == RobustKernel.NONE
    g.setVoxelResolution(res)
    g.setNeighborSearchMethod(NeighborSearchMethod.DIRECT7)
    g.setRobustKernel(RobustKernel.CAUCHY, width)
    g.setInputSource(w.source); g.setInputTarget(w.target)
    g.align()
    T_cpp = np.array([float.fromhex(v) for v in rows["T"]], np.float32).reshape(4, 4).T
    assert np.array_equal(T_cpp, g.getFinalTransformation())
    assert [int(rows["converged"][0]), int(rows["converged"][2])] == [int(g.hasConverged()), g.nr_iterations_]
    s, wt = g.robust_terms()
    n = len(w.source)
    assert s.shape == wt.shape == (n, 7) and [int(v) for v in rows["terms"]] == [n * 7, n * 7]
    both = np.fromfile(terms_path, np.float64)
    assert np.array_equal(both[:n * 7].reshape(n, 7), s) and np.array_equal(both[n * 7:].reshape(n, 7), wt)
    assert ((wt > 0) & (wt < 1)).any() and (s == -1).any()
    g.setRobustKernel(RobustKernel.NONE)
    g.align()
    assert not np.array_equal(g.getFinalTransformation(), T_cpp)  # the kernel did something
    g.close()
