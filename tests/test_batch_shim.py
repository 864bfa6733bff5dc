"""The batch surface of the C++ shim (include/nano_gicp/nano_gicp.hpp): alignBatch(guesses) and getFitnessScores(transforms), compiled
with g++ -Wall -Werror (tests/cpp/batch_shim.cpp) and, on the GPU, compared bit for bit with the shim's own align() in a loop on the
golden fixture."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "batch_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "batch_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_batch_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_shim_batch_matches_its_own_align_loop(hip_lib, golden, tmp_path):
    from direct_lidar_odometry_amd import clouds
    src, tgt = golden["source"], golden["target"]
    guesses = [np.eye(4), clouds.make_pose((0.05, -0.03, 0.02), (0.2, -0.3, 0.5)), clouds.make_pose((0.2, 0.1, 0.0), (0, 0, 3.0)),
               clouds.make_pose((-0.1, 0.3, 0.05), (1.0, 0, -8.0)), clouds.make_pose((2.0, 0, 0))]
    paths = []
    for name, a in (("src", src[:, :3]), ("tgt", tgt[:, :3]), ("guesses", np.stack([g.T.reshape(16) for g in guesses]))):
        p = tmp_path / f"{name}.bin"
        np.ascontiguousarray(a, np.float32).tofile(p)
        paths.append(str(p))
    exe = _build(tmp_path)
    res = subprocess.run([exe, *paths, repr(float(golden["max_corr_dist"])), "0.04"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stderr)
    rows = {"batch": {}, "loop": {}}
    for line in res.stdout.splitlines():
        tag, *vals = line.split()
        if tag == "untouched":
            assert vals == ["1"]
        else:
            rows[tag][int(vals[0])] = vals[1:]
    assert sorted(rows["batch"]) == sorted(rows["loop"]) == list(range(len(guesses)))
    for lane in range(len(guesses)):
        assert rows["batch"][lane] == rows["loop"][lane], lane
    assert len({tuple(v) for v in rows["batch"].values()}) > 1  # the guesses do not all end alike
