"""The pose graph through the C++ shim (include/nano_gicp/nano_gicp.hpp: poseGraphAddNodes / AddEdges / Optimize / Poses / Corrections,
edgeFromAlignment ...), compiled with g++ -Wall -Werror (tests/cpp/pose_graph_shim.cpp) and, on the GPU, compared byte for byte with the
Python API on the same graph (the optimiser is deterministic)."""
import os
import subprocess

import numpy as np
import pytest

import _pose_graph_cases as pc
import _pose_graph_model as pgm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ngicp_pose_graph_clear", "ngicp_pose_graph_size", "ngicp_pose_graph_add_nodes", "ngicp_pose_graph_add_edges", "ngicp_pose_graph_get_edges",
         "ngicp_pose_graph_set_fixed", "ngicp_pose_graph_get_fixed", "ngicp_pose_graph_set_robust", "ngicp_pose_graph_get_poses", "ngicp_pose_graph_set_poses",
         "ngicp_pose_graph_linearize", "ngicp_pose_graph_multiply", "ngicp_pose_graph_optimize", "ngicp_pose_graph_corrections", "ngicp_pose_graph_kernel_ms"]
METHODS = ["poseGraphClear", "poseGraphSize", "poseGraphAddNodes", "poseGraphAddEdges", "poseGraphSetFixed", "poseGraphSetRobust", "poseGraphPoses",
           "poseGraphSetPoses", "poseGraphLinearize", "poseGraphMultiply", "poseGraphOptimize", "poseGraphCorrections", "poseGraphKernelMs", "edgeFromAlignment"]


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "pose_graph_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_graph_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_python_api_the_header_and_the_shim_declare_the_entries():
    from direct_lidar_odometry_amd import nano_gicp
    assert all(n in nano_gicp.EXPORTS for n in NAMES)
    header = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    assert all(f"int {n}(" in header for n in NAMES)
    shim = open(os.path.join(ROOT, "include", "nano_gicp", "nano_gicp.hpp")).read()
    for m in METHODS:
        assert callable(getattr(nano_gicp.NanoGICP, m)) and f" {m}(" in shim, m
    for n in NAMES:
        assert f"{n}(h_" in shim, n


def test_pose_graph_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


def test_the_python_edge_from_alignment_is_the_model_s():
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP
    rng = np.random.default_rng(9)
    A = rng.normal(size=(6, 6))
    H = A @ A.T + np.eye(6)
    Ti, Ta = pgm.make_pose(rng.uniform(-1, 1, 3), rng.uniform(-80, 80, 3)), pgm.make_pose(rng.uniform(-1, 1, 3), rng.uniform(-80, 80, 3))
    Z, Lam = NanoGICP.edgeFromAlignment(Ti, Ta, H)
    Zm, Lm = pgm.edge_from_alignment(Ti, Ta, H)
    assert np.abs(Z - Zm).max() <= 1e-12 * np.abs(Zm).max() and np.abs(Lam - Lm).max() <= 1e-12 * np.abs(Lm).max()
    assert np.array_equal(Lam, Lam.T) and np.array_equal(Z[3], [0.0, 0.0, 0.0, 1.0])


@pytest.mark.gpu
def test_pose_graph_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP
    g, _ = pc.false_edge(pgm.CAUCHY)
    n, m = g.n, g.m
    pad = b"\0" * ((8 - n % 8) % 8)
    blob = b"".join([np.array([n, m], np.int64).tobytes(), np.ascontiguousarray(g.poses.transpose(0, 2, 1)).tobytes(), g.fixed.astype(np.uint8).tobytes(), pad,
                     g.ij.astype(np.int32).tobytes(), np.ascontiguousarray(g.Z.transpose(0, 2, 1)).tobytes(), np.ascontiguousarray(g.info).tobytes(),
                     g.flags.astype(np.uint8).tobytes()])
    path = tmp_path / "graph.bin"
    path.write_bytes(blob)
    exe = _build(tmp_path)
    out = subprocess.run([exe, str(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines()}

    e = NanoGICP()
    assert [e.poseGraphAddNodes(g.poses, g.fixed), e.poseGraphAddEdges(g.ij, g.Z, g.info, g.flags)] == [0, 0]
    assert rows["added"] == ["0", "0", str(n), str(m)]
    assert rows["refused"] == ["-1", str(n), str(m)] and "self-edge" in out.stderr
    e.poseGraphSetRobust(pgm.CAUCHY, 3.0)
    chi2 = e.poseGraphLinearize()["chi2"]
    res = e.poseGraphOptimize(**pc.OPTIONS)
    want = ["1", res["iterations"], res["accepted"], res["cg_iterations"], int(res["converged"]), len(res["trace"]), repr(chi2), repr(res["initial_chi2"]),
            repr(res["final_chi2"])]
    assert rows["optimize"][:6] == [str(v) for v in want[:6]]
    assert [float(v) for v in rows["optimize"][6:]] == [chi2, res["initial_chi2"], res["final_chi2"]]
    assert res["accepted"] >= 2
    poses = np.fromfile(tmp_path / "poses.bin", np.float64).reshape(n, 4, 4).transpose(0, 2, 1)
    assert np.ascontiguousarray(poses).tobytes() == e.poseGraphPoses().tobytes()
    Cs = np.fromfile(tmp_path / "corrections.bin", np.float32).reshape(n, 4, 4).transpose(0, 2, 1)
    assert np.ascontiguousarray(Cs).tobytes() == e.poseGraphCorrections(np.arange(n)).tobytes()
    assert rows["corrections"] == ["1", str(n), "1"] and rows["cleared"] == ["0", "0"]
    H = np.array([[(50.0 + 7.0 * a if a == b else 0.0) + 0.5 * (a + b) for b in range(6)] for a in range(6)])
    Z, Lam = NanoGICP.edgeFromAlignment(g.poses[0], g.poses[1], H)
    got = np.array([float(v) for v in rows["edge"]])
    Zc, Lc = got[:16].reshape(4, 4).T, got[16:].reshape(6, 6)
    assert np.abs(Zc - Z).max() <= 1e-12 * np.abs(Z).max() and np.abs(Lc - Lam).max() <= 1e-12 * np.abs(Lam).max() and np.array_equal(Lc, Lc.T)
    e.close()
