"""The process-wide kernel variants, each in a child process of its own, under the per-pass oracle check (-m gpu).

NGICP_PASS_IMPL, NGICP_FUSED, NGICP_QUEUE, NGICP_ORDER and NGICP_PASS_WPS are read once per process (csrc/ngicp_route.h:
read_process_switches, behind switches()'s static), so monkeypatch cannot reach them: every variant runs tests/_variant_worker.py in a fresh child, one
at a time, on the 10k scan-to-scan cases, two adversarial shapes and c3 FIXED20.  Without NGICP_PASS_WPS the grid size picks the
3- or 4-waves-per-SIMD build (nblocks > 2 * pass_slots), so a workload meets only one of them: each variant also runs with each build
forced.  Left out on purpose: NGICP_PERSIST_COOP=0 and NGICP_PERSIST_ONE (timing only; their blocks wait for each other without a
cooperative launch) and NGICP_DEBUG_MODE (meaningless results by design).

A child that dies by a signal or runs past its time limit stops the module: the remaining children are skipped, naming it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_variant_worker.py")

CASES = ["dlo_s2s", "fixed20", "gauss_newton", "lm_rejection", "one_iteration", "lines", "clumps", "c3_fixed20"]
# wall-time allowance per case: well above a normal run, and above the engine's own 30 s wait for a pass, so that a stall is
# reported by the engine (an error, non-zero exit) before the child is killed
BUDGET_S = {"c3_fixed20": 300}
BUDGET_DEFAULT_S = 90

VARIANTS = {
    "wps3": {"NGICP_PASS_WPS": "3"},
    "wps4": {"NGICP_PASS_WPS": "4"},
    "staged-wps3": {"NGICP_PASS_IMPL": "1", "NGICP_PASS_WPS": "3"},
    "staged-wps4": {"NGICP_PASS_IMPL": "1", "NGICP_PASS_WPS": "4"},
    "fused-wps3": {"NGICP_FUSED": "1", "NGICP_PASS_WPS": "3"},
    "fused-wps4": {"NGICP_FUSED": "1", "NGICP_PASS_WPS": "4"},
    "queue-wps3": {"NGICP_QUEUE": "1", "NGICP_PASS_WPS": "3"},
    "queue-wps4": {"NGICP_QUEUE": "1", "NGICP_PASS_WPS": "4"},
    "xcd-order": {"NGICP_ORDER": "xcd"},
}

SWITCHES = ("NGICP_PASS_IMPL", "NGICP_FUSED", "NGICP_QUEUE", "NGICP_ORDER", "NGICP_PASS_WPS")  # what the variants set; nothing else is touched
_stopped = []  # the child that died by a signal or timed out: nothing more is started after it


@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_pass_under_process_variant(hip_lib, oracle_mod, name):
    if _stopped:
        pytest.skip(f"not started: the child of variant {_stopped[0]} ended abnormally")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}  # (NGICP_LIB and the per-handle switches pass through)
    env.update(VARIANTS[name])
    timeout = 60 + sum(BUDGET_S.get(c, BUDGET_DEFAULT_S) for c in CASES)
    try:
        res = subprocess.run([sys.executable, WORKER, *CASES], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _stopped.append(name)
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"{name}: no result after {timeout} s\n{out[-3000:]}")
    if res.returncode < 0:
        _stopped.append(name)
    assert res.returncode == 0, f"{name} ({VARIANTS[name]}): exit {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    print(name, json.dumps(out["cases"]))
    assert out["variant"] == VARIANTS[name]
    assert sorted(out["cases"]) == sorted(CASES) and all(c["passes"] >= 1 for c in out["cases"].values())
