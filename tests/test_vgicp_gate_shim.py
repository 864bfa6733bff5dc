"""The gated insert through the C++ shim (include/nano_gicp/nano_gicp.hpp: insertIntoVoxelMapGated / voxelMapInsertClasses / InsertClass),
compiled with g++ -Wall -Werror (tests/cpp/vgicp_gate_shim.cpp) and, on the GPU, compared byte for byte with the Python API on the same
clouds: the classes, the counts, the map behind a dry run and behind the insert, and a refusal."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ngicp_voxel_rolling_insert_gated", "ngicp_voxel_rolling_insert_classes"]


def _build(out_dir):
    libdir = os.path.join(ROOT, "direct_lidar_odometry_amd")
    exe = os.path.join(str(out_dir), "vgicp_gate_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vgicp_gate_shim.cpp"),
           "-o", exe, "-L" + libdir, "-lngicp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_vgicp_gate_shim_compiles(hip_lib, tmp_path):
    assert os.path.exists(_build(tmp_path))


def test_header_python_and_shim_declare_the_gate_entries(hip_lib):
    from direct_lidar_odometry_amd import nano_gicp
    assert all(n in nano_gicp.EXPORTS for n in NAMES) and all(hasattr(hip_lib, n) for n in NAMES)
    header = open(os.path.join(ROOT, "include", "ngicp.h")).read()
    assert all(f"int {n}(" in header for n in NAMES)
    assert "typedef struct ngicp_gate_options" in header and "typedef struct ngicp_gate_result" in header and "rolling voxel map: gated insert" in header
    shim = open(os.path.join(ROOT, "include", "nano_gicp", "nano_gicp.hpp")).read()
    assert all(f"{n}(h_" in shim for n in NAMES) and "enum InsertClass" in shim
    for m in ("insertIntoVoxelMapGated", "voxelMapInsertClasses"):
        assert callable(getattr(nano_gicp.NanoGICP, m)) and m in shim
    # the Python mirror of the options has the header's fields, in its order, with its defaults; the classes have the header's values
    fields = [f for f, _ in nano_gicp.GateOptions._fields_]
    assert fields == ["max_mahalanobis", "min_voxel_count", "insert_new", "insert_unjudged", "dry_run"]
    struct = header[header.index("typedef struct ngicp_gate_options"):header.index("} ngicp_gate_options;")]
    at = [struct.index(f" {f};") for f in fields]
    assert at == sorted(at)
    assert nano_gicp.GateOptions.DEFAULTS == dict(min_voxel_count=1, insert_new=1, insert_unjudged=1, dry_run=0)
    for name, value in (("NEW", 0), ("EXPLAINED", 1), ("CONFLICT", 2), ("UNJUDGED", 3)):
        assert f"#define NGICP_GATE_{name} {value}" in header and getattr(nano_gicp, f"GATE_{name}") == value and f"INSERT_{name} = NGICP_GATE_{name}" in shim
    assert [f for f, _ in nano_gicp.GateResult._fields_] == ["n_points", "n_class", "n_kept", "n_new", "n_touched", "kernel_ms"]


@pytest.mark.gpu
def test_vgicp_gate_shim_matches_python_api(hip_lib, tmp_path):
    from direct_lidar_odometry_amd import clouds
    from direct_lidar_odometry_amd.nano_gicp import NanoGICP, NgicpError
    sc = clouds.make_scene()
    t = (0.75, -0.5, 0.125)  # (exact in float: the shim parses them from text)
    scans = [clouds.vlp16(sc, clouds.make_pose(p, (0.0, 0.0, 0.0)), 400 + i, cols=100) for i, p in enumerate(((0.0, 0.0, 0.0), t))]
    res, gate = 1.0, 0.5
    paths = []
    for i, a in enumerate(scans):
        p = tmp_path / f"scan{i}.bin"
        np.ascontiguousarray(a[:, :3], np.float32).tofile(p)
        paths.append(str(p))
    exe = _build(tmp_path)
    out = subprocess.run([exe, repr(res), repr(gate), *[repr(v) for v in t], *paths], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    rows = {l[0]: l[1:] for l in lines}
    ints = lambda tag, dt=np.int64: np.array([int(v) for v in rows[tag]], dt)
    hexes = lambda tag: np.array([float.fromhex(v) for v in rows[tag]])

    def same_map(tag, g):
        ijk, s, c, cnt, st = g.rollingVoxelMap()
        assert [int(v) for v in rows[tag + "_n"]] == [len(ijk), g.voxelRollingStats()["inserts"]]
        assert np.array_equal(ints(tag + "_ijk"), ijk.reshape(-1)) and np.array_equal(ints(tag + "_count"), cnt) and np.array_equal(ints(tag + "_stamp"), st)
        assert hexes(tag + "_sum").tobytes() == s.tobytes()
        assert hexes(tag + "_covsum").tobytes() == np.ascontiguousarray(c.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]]).tobytes()

    def same_classes(tag, g):
        cls = g.voxelMapInsertClasses()
        assert rows[tag + "_ok"] == ["1", str(len(cls))] and np.array_equal(ints(tag + "_cls", np.uint8), cls)

    def result_row(r):
        return ["1", str(r["n_points"]), *map(str, r["n_class"]), str(r["n_kept"]), str(r["n_new"]), str(r["n_touched"]), "1"]

    g = NanoGICP()
    g.setVoxelResolution(res); g.setNeighborSearchMethod(7); g.setVoxelRolling(True)
    assert rows["before_ok"] == ["0", "0"]
    with pytest.raises(NgicpError):
        g.voxelMapInsertClasses()
    T = np.eye(4, dtype=np.float32)
    g.setInputSource(scans[0])
    assert rows["insert"] == ["1", *map(str, g.insertIntoVoxelMap(g, T))]
    g.setInputSource(scans[1])
    T[:3, 3] = t
    dry = g.insertIntoVoxelMapGated(g, T, gate, dry_run=1)
    assert rows["dry"] == result_row(dry) and (dry["n_new"], dry["n_touched"]) == (0, 0)
    assert dry["n_class"][1] > 0 and dry["n_class"][2] > 0  # (the scan has points of both kinds under this gate)
    same_classes("dry", g)
    with pytest.raises(NgicpError) as e:
        g.insertIntoVoxelMapGated(g, T, gate, dry_run=1, min_voxel_count=0)
    assert e.value.code == -2 and rows["refused"] == ["0"] + ["0"] * 8 + ["1"]
    same_classes("refused", g)  # the refusal left the dry run's classes readable, on both sides
    assert rows["refused_cls"] == rows["dry_cls"]
    same_map("kept", g)
    real = g.insertIntoVoxelMapGated(g, T, gate, min_voxel_count=2, insert_unjudged=0)
    assert rows["gated"] == result_row(real) and 0 < real["n_kept"] < real["n_points"] and real["n_touched"] > 0
    same_classes("gated", g)
    same_map("inserted", g)
    assert int(rows["inserted_n"][1]) == int(rows["kept_n"][1]) + 1
    g.close()
