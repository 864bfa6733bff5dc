"""The pose graph's planning header (direct_lidar_odometry_amd/csrc/ngicp_pose_graph_plan.h: caps, refusals, the union-find component
check, the per-node incidence lists) compiled into a stand-alone program with its own main (tests/cpp/pose_graph_plan.cpp; g++ -std=c++17
-Wall -Werror against the header alone - no library, no GPU) and held to the numpy model (tests/_pose_graph_model.py); once more under
AddressSanitizer and UBSan."""
import os
import subprocess

import numpy as np
import pytest

import _pose_graph_cases as pc
import _pose_graph_model as pgm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CAP, M_CAP = pgm.MAX_NODES, pgm.MAX_EDGES


def _graphs():
    """(n, fixed, pairs)"""
    rng = np.random.default_rng(5)
    out = [(0, [], []), (1, [0], []), (1, [1], []), (3, [0, 0, 0], [])]
    out.append((11, [0, 0, 1] + [0] * 8, pc.chain_pairs(6) + [(5, 0)] + [(a, a + 1) for a in range(6, 10)]))  # two components, one without a fixed node
    out.append((131, [0, 1] + [0] * 129, [(0, a) if a % 2 else (a, 0) for a in range(1, 131)]))                # a hub with 130 edges
    out.append((4, [1, 0, 0, 0], [(0, 1), (0, 1), (1, 0), (1, 2), (3, 2), (0, 3), (1, 0)]))                    # multi-edges, reversed edges
    out.append((6, [0, 0, 0, 0, 0, 1], [(5, 4), (4, 3), (3, 2), (2, 1), (1, 0)]))                             # a chain given backwards
    out.append((7, [0, 0, 0, 1, 0, 0, 0], [(0, 1), (2, 3), (5, 6)]))                                           # four components, three ungauged
    n = 300
    pairs = [tuple(int(v) for v in rng.choice(n, 2, replace=False)) for _ in range(500)]
    out.append((n, list((rng.random(n) < 0.02).astype(int)), pairs))
    return out


def _expected_graph(n, fixed, pairs):
    off, ent = pgm.csr(n, np.array(pairs, np.int64).reshape(-1, 2))
    k = pgm.ungauged_components(n, np.array(pairs, np.int64).reshape(-1, 2), np.array(fixed, bool))
    return "csr" + "".join(f" {v}" for v in off) + " ;" + "".join(f" {v}" for v in ent) + f" ; ungauged {k}"


def _pose(bad):
    T = np.eye(4)
    T[:3, 3] = [3.0, -2.0, 0.5]
    if bad == 1:
        T[1, 2] = np.nan
    if bad == 2:
        T[3, 1] = 1e-300
    return T


def _info(bad):
    L = np.array([[(4.0 if a == b else 0.0) + 0.125 * (a + b) for b in range(6)] for a in range(6)])
    if bad == 1:
        L[2, 4] += 1e-15
    if bad == 2:
        L[5, 5] = np.inf
    return L


def _node_calls():
    """(n_now, count, [bad per listed node])"""
    return [(0, 1, [0]), (5, 3, [0, 0, 0]), (5, 3, [0, 1, 0]), (5, 3, [0, 0, 2]), (0, 0, []), (N_CAP - 1, 1, [0]), (N_CAP, 1, [0]), (N_CAP - 2, 3, [0, 0, 0]),
            (0, N_CAP + 1, [0]), (N_CAP - 3, 3, [0, 0, 0])]


def _edge_calls():
    """(n_nodes, m_now, count, [(i, j, zbad, ibad) per listed edge])"""
    return [(4, 0, 1, [(0, 1, 0, 0)]), (4, 7, 2, [(0, 1, 0, 0), (3, 2, 0, 0)]), (4, 0, 1, [(2, 2, 0, 0)]), (4, 0, 1, [(0, 4, 0, 0)]), (4, 0, 1, [(-1, 2, 0, 0)]),
            (4, 0, 1, [(0, 1, 1, 0)]), (4, 0, 1, [(0, 1, 2, 0)]), (4, 0, 1, [(0, 1, 0, 1)]), (4, 0, 1, [(0, 1, 0, 2)]), (4, 0, 0, []),
            (4, 0, 3, [(0, 1, 0, 0), (1, 2, 0, 0), (3, 3, 0, 0)]),  # all or nothing: the last one spoils the call
            (4, M_CAP - 1, 1, [(0, 1, 0, 0)]), (4, M_CAP, 1, [(0, 1, 0, 0)]), (4, M_CAP - 1, 2, [(0, 1, 0, 0), (1, 2, 0, 0)]), (4, 0, M_CAP + 1, [(0, 1, 0, 0)]),
            (0, 0, 1, [(0, 1, 0, 0)])]


def _expected_nodes(n_now, count, bad):
    T = np.array([_pose(b) for b in bad]).reshape(-1, 4, 4) if len(bad) == count else np.broadcast_to(np.eye(4), (count, 4, 4))
    try:
        pgm.check_add_nodes(n_now, T)
        return "ok"
    except pgm.Refused:
        return "refused"


def _expected_edges(n_nodes, m_now, count, listed):
    if len(listed) == count:
        ij, Z, L = [(e[0], e[1]) for e in listed], [_pose(e[2]) for e in listed], [_info(e[3]) for e in listed]
        args = (np.array(ij, np.int64).reshape(-1, 2), np.array(Z).reshape(-1, 4, 4), np.array(L).reshape(-1, 6, 6))
    else:
        args = (np.zeros((count, 2), np.int64), np.broadcast_to(np.eye(4), (count, 4, 4)), np.broadcast_to(np.eye(6), (count, 6, 6)))
    try:
        pgm.check_add_edges(n_nodes, m_now, *args)
        return "ok"
    except pgm.Refused:
        return "refused"


@pytest.mark.parametrize("name,extra", [("pose_graph_plan", []), ("pose_graph_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_the_planning_header_matches_the_model(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "cpp", "pose_graph_plan.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines, want = [], []
    for n, fixed, pairs in _graphs():
        lines.append(" ".join(str(v) for v in ["graph", n, len(pairs), *fixed, *[x for p in pairs for x in p]]))
        want.append(_expected_graph(n, fixed, pairs))
    for n_now, count, bad in _node_calls():
        lines.append(" ".join(str(v) for v in ["nodes", n_now, count, len(bad), *bad]))
        want.append(_expected_nodes(n_now, count, bad))
    for n_nodes, m_now, count, listed in _edge_calls():
        lines.append(" ".join(str(v) for v in ["edges", n_nodes, m_now, count, len(listed), *[x for e in listed for x in e]]))
        want.append(_expected_edges(n_nodes, m_now, count, listed))
    path = os.path.join(str(tmp_path), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    got = run.stdout.splitlines()
    assert got[-1] == f"cases {len(want)}"
    assert got[:-1] == want
    assert want.count("ok") >= 6 and want.count("refused") >= 14           # every kind of answer occurred
    assert any(w.endswith("ungauged 0") for w in want) and any(w.endswith("ungauged 1") for w in want) and any(w.endswith("ungauged 3") for w in want)


def test_the_model_s_lists_are_the_incident_edges_in_ascending_order():
    n, _, pairs = _graphs()[-1]
    off, ent = pgm.csr(n, np.array(pairs))
    assert off[0] == 0 and off[-1] == 2 * len(pairs) and sorted(ent) == list(range(2 * len(pairs)))
    for k in range(n):
        mine = ent[off[k]:off[k + 1]]
        assert list(mine) == sorted(mine)
        assert all(pairs[v // 2][v % 2] == k for v in mine)
    root = pgm.components(n, np.array(pairs))
    for a, b in pairs:
        assert root[a] == root[b]
