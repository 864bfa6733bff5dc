"""The route table (direct_lidar_odometry_amd/csrc/ngicp_route.h) against the decision code it replaced: tests/cpp/route_table.cpp carries
that code as legacy_* functions, walks the whole cross product of switches and facts, and checks the two switch readers' parsing and clamps
through a fake lookup.  Compiled with g++ -std=c++17 -Wall -Werror against the header alone - no library, no GPU - and run; once more under
AddressSanitizer and UBSan (a stand-alone program with its own main)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(out_dir, name, extra):
    exe = os.path.join(str(out_dir), name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "cpp", "route_table.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    return res


@pytest.mark.parametrize("name,extra", [("route_table", []), ("route_table_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_route_table_matches_the_code_it_replaced(tmp_path, name, extra):
    res = _build_and_run(tmp_path, name, extra)
    words = res.stdout.split()
    got = dict(zip(words[0::2], map(int, words[1::2])))
    assert got["mismatches"] == 0
    assert got["cells"] > 4_000_000  # the whole cross product was walked
    assert got["new_refusals"] > 0   # ... and met the one deliberate change: a robust kernel under NGICP_PERSIST_ONE
    assert res.stderr == ""
