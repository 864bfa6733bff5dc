"""The scan context entries on the host side: the public header, the Python API's export list and methods and the C++ shim
(include/nano_gicp/nano_gicp.hpp) all declare them, and the shim's use of them (tests/cpp/scan_context_shim.cpp) compiles with
g++ -Wall -Werror.  The program's run against the Python API is in tests/test_gpu_scan_context.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ngicp_scan_context_set_params", "ngicp_scan_context_get_params", "ngicp_scan_context_tables", "ngicp_scan_context_compute",
         "ngicp_scan_context_add", "ngicp_scan_context_add_descriptor", "ngicp_scan_context_count", "ngicp_scan_context_get",
         "ngicp_scan_context_clear", "ngicp_scan_context_distances", "ngicp_scan_context_match", "ngicp_scan_context_kernel_ms"]
METHODS = ["setScanContextParams", "getScanContextParams", "scanContextTables", "computeScanContext", "addScanContext", "addScanContextDescriptor",
           "numScanContexts", "scanContext", "clearScanContexts", "scanContextDistances", "matchScanContext", "scanContextGuess"]


def test_header_exports_python_and_shim_declare_the_scan_context_entries():
    from direct_lidar_odometry_amd import nano_gicp
    assert all(n in nano_gicp.EXPORTS for n in NAMES)
    header = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    assert all(f"int {n}(" in header for n in NAMES)
    assert "scan context" in header and "outside implementation is claimed" in header
    for m in METHODS:
        assert callable(getattr(nano_gicp.NanoGICP, m)), m
    shim = open(os.path.join(ROOT, "include", "nano_gicp", "nano_gicp.hpp")).read()
    assert "struct ScanContextMatch {" in shim
    for field in ("int id;", "double distance;", "int shift;"):
        assert field in shim.split("struct ScanContextMatch {")[1].split("};")[0]
    for m in METHODS:
        assert f" {m}(" in shim, m
    # the entries beside it are as they were
    assert "float medianRange(int which = 0)" in shim and "VoxelFitness getVoxelFitness(" in shim


def test_the_library_exports_the_entries(hip_lib):
    for n in NAMES:
        assert hasattr(hip_lib, n), n


def test_the_kernels_are_in_the_source():
    src = open(os.path.join(ROOT, "direct_lidar_odometry_amd", "csrc", "ngicp_scan_context.h")).read()
    for k in ("k_sc_build", "k_sc_norms", "k_sc_match", "k_sc_topk"):
        assert f" {k}(" in src, k
    api = open(os.path.join(ROOT, "direct_lidar_odometry_amd", "csrc", "ngicp_api.hip")).read()
    assert '#include "ngicp_scan_context.h"' in api


def test_scan_context_shim_compiles(hip_lib, tmp_path):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(tmp_path), "scan_context_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "scan_context_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert os.path.exists(exe)
