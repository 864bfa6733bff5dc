"""Moving keyframes through the C++ shim (include/nano_gicp/nano_gicp.hpp: transformKeyframes / getKeyframe / keyframeTransformKernelMs),
compiled with g++ -Wall -Werror (tests/cpp/keyframe_move_shim.cpp) and, on the GPU, compared byte for byte with the Python API on the
same clouds."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ngicp_keyframe_get", "ngicp_keyframe_transform", "ngicp_keyframe_transform_kernel_ms"]
METHODS = ["getKeyframe", "transformKeyframes", "keyframeTransformKernelMs"]


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "keyframe_move_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "keyframe_move_shim.cpp"),
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


def test_keyframe_move_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


def _pose(x, y, z, c, s):
    T = np.eye(4, dtype=np.float32)
    T[0, 0] = T[1, 1] = np.float32(c)
    T[1, 0] = np.float32(s)
    T[0, 1] = -np.float32(s)
    T[:3, 3] = np.float32(x), np.float32(y), np.float32(z)
    return T


def _read(path):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw, np.int64, 1)[0])
    pts = np.frombuffer(raw, np.float32, n * 3, 8).reshape(n, 3)
    covs = np.frombuffer(raw, np.float64, n * 16, 8 + n * 12).reshape(n, 4, 4).transpose(0, 2, 1)
    assert 8 + n * 12 + n * 128 == len(raw)
    return pts, covs


@pytest.mark.gpu
def test_keyframe_move_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP, NgicpError
    rng = np.random.default_rng(21)
    kfs = [(rng.uniform(-12, 12, (n, 3)) + [4.0 * i, 0, 0]).astype(np.float32) for i, n in enumerate((400, 65, 1030))]
    Ts = np.stack([np.eye(4, dtype=np.float32), _pose(0.5, -0.25, 0.125, 0.96, 0.28), _pose(-3.0, 1.5, 0.0, 0.6, -0.8)])
    paths = []
    for i, a in enumerate(kfs):
        p = tmp_path / f"in{i}.bin"
        a.tofile(p)
        paths.append(str(p))
    np.ascontiguousarray(Ts.transpose(0, 2, 1)).tofile(tmp_path / "T.bin")
    exe = _build(tmp_path)
    out = subprocess.run([exe, str(tmp_path), str(tmp_path / "T.bin"), *paths], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines()}

    prod, g = NanoGICP(), NanoGICP()
    for a in kfs:
        prod.setInputSource(a)
        prod.calculateSourceCovariances()
        g.addKeyframe(prod)
    assert rows["submap"] == [str(int(g.setSubmapKeyframes([0, 1])))] == ["1"]
    stale = g.transformKeyframes([2, 1], Ts[[2, 1]])
    assert rows["moved"] == ["1", str(int(stale)), "1"] and stale is True and g.keyframeTransformKernelMs() > 0.0
    assert rows["submap_again"] == [str(int(g.setSubmapKeyframes([0, 1])))] == ["1"]
    with pytest.raises(NgicpError, match="positions 0 and 1"):
        g.transformKeyframes([0, 0], Ts[[2, 2]])
    assert rows["refused"] == ["0", "0"] and "positions 0 and 1" in out.stderr
    assert rows["submap_after_refusal"] == [str(int(g.setSubmapKeyframes([0, 1])))] == ["0"]
    for i in range(3):
        pts, covs = _read(tmp_path / f"kf{i}.bin")
        got_p, got_c = g.getKeyframe(i)
        assert pts.tobytes() == got_p.tobytes() and np.ascontiguousarray(covs).tobytes() == got_c.tobytes(), f"keyframe {i}"
    assert np.array_equal(g.getKeyframe(0)[0], kfs[0]) and not np.array_equal(g.getKeyframe(2)[0], kfs[2])
    prod.close(); g.close()
