"""The pose prior through the C++ shim (include/nano_gicp/nano_gicp.hpp: setPosePrior, clearPosePrior, getPosePrior, posePriorTerms),
compiled with g++ against the C ABI (tests/cpp/pose_prior_shim.cpp) and checked against the Python host bit for bit on the exact route."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "pose_prior_shim")


def _build(hip_lib):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_prior_shim.cpp"),
           "-o", BIN, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return BIN


def test_the_shim_program_compiles(hip_lib):
    assert os.path.exists(_build(hip_lib))


@pytest.mark.gpu
def test_the_shim_equals_the_python_host_bit_for_bit(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds, nano_gicp
    exe = _build(hip_lib)
    w = clouds.scan_to_scan(2000)
    Tp = clouds.make_pose((0.05, -0.04, 0.02), (0.5, -0.3, 1.0)) @ np.asarray(w.guess, np.float64)
    A = np.random.default_rng(4).normal(size=(6, 6))
    Lam = 2e3 * (A @ A.T)
    Te = clouds.make_pose((0.02, 0.01, -0.03), (1.0, 2.0, -1.5)) @ Tp
    guess = np.asarray(w.guess, np.float32)
    np.ascontiguousarray(w.source, np.float32).tofile(tmp_path / "src.bin")
    np.ascontiguousarray(w.target, np.float32).tofile(tmp_path / "tgt.bin")
    np.r_[Tp.T.ravel(), Lam.T.ravel(), guess.astype(np.float64).T.ravel(), Te.T.ravel()].tofile(tmp_path / "params.bin")
    res = subprocess.run([exe, str(tmp_path / "src.bin"), str(tmp_path / "tgt.bin"), str(tmp_path / "params.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "pose prior" in res.stderr  # the bad prior was reported
    out = np.fromfile(tmp_path / "out.bin")
    assert out.shape == (16 + 36 + 2 + 1 + 16 + 36 + 6 + 1 + 36 + 6 + 4,)

    g = nano_gicp.NanoGICP()
    g.setMaxCorrespondenceDistance(1.0)
    g.setInputSource(w.source); g.setInputTarget(w.target)
    g.align(guess)
    T_plain = g.getFinalTransformation().copy()
    g.setPosePrior(Tp, Lam)
    g.align(guess)
    T = g.getFinalTransformation()
    assert not np.array_equal(T, T_plain)
    r, c, Hp, b = g.pose_prior_terms(Te)
    at = 0

    def take(n):
        nonlocal at
        at += n
        return out[at - n:at]

    assert np.array_equal(take(16).reshape(4, 4).T, T.astype(np.float64))
    assert np.array_equal(take(36).reshape(6, 6).T, g.getFinalHessian())
    assert tuple(take(2)) == (g.nr_iterations_, float(g.converged_))
    assert take(1)[0] == 1.0 and np.array_equal(take(16).reshape(4, 4).T, Tp) and np.array_equal(take(36).reshape(6, 6).T, Lam)
    assert np.array_equal(take(6), r) and take(1)[0] == c and np.array_equal(take(36).reshape(6, 6).T, Hp) and np.array_equal(take(6), b)
    assert tuple(take(4)) == (0.0, 1.0, 0.0, 0.0)  # the bad prior refused, the former one kept; after clearPosePrior: no terms, no prior
    g.close()
