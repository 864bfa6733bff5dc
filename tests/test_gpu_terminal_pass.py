"""K4-only passes (-m gpu): a pass whose linearisation can never be adopted evaluates only the trial's error (DESIGN.md 4.1,
LmHot::lin_unneeded, ngicp_lm.h set_lin_unneeded), and nothing an alignment leaves may tell.

Every scenario runs in two fresh child processes (tests/_terminal_pass_worker.py; the switch is read at ngicp_create), one as built and
one with NGICP_FULL_LAST_PASS=1, which makes every pass search and linearise as before.  Bit-equal between the two: the final
transformation, the final Hessian, `converged`, nr_iterations_, the LM trace, correspondences() (indices and squared distances),
the error at the final pose term by term (robust_terms: e^T M e from the persisted correspondences and Mahalanobis matrices;
ngicp_compute_error itself wants a linearize hook first, which would replace the state in question), and `passes`.
search_passes == passes with the switch and < passes without (Gauss-Newton: equal either way, the word is never set).

Shapes: 2 000 source points against 5 000 (fewer batches than a full group in the last block, a partial batch) and the 10 000 against
10 000 of the parity tests.

The launch order (test_two_alignments_in_a_row).  The order is a counting sort of MEASURED block durations: no two runs of the same
binary produce the same buffer, so "the same order with and without the switch" cannot be asked for bit by bit.  What is asked instead
pins the two ways a K4-only pass could spoil it, on the buffers read back after the first alignment (NGICP_DEBUG_COSTS):
  * the order is exactly the solver's sort of the costs in the cost buffer (both were left by the same pass: a K4-only pass that stored
    its costs while the solver kept the old order, or the reverse, breaks this);
  * those costs are a searching pass's: their sum lies within a factor of two of the sum the other mode measured.  The two sums come
    from two warm late passes of the same alignment (the last and the last but one); a K4-only pass does a quarter of a pass's work
    (search and linearisation are three quarters of a launch), so its costs would fall below half.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_terminal_pass_worker.py")
SHAPES = ("2k_5k", "10k_10k")
BIT_EQUAL = ("T", "H", "converged", "iters", "trace", "corr", "sqd", "err", "terms", "passes")
REJECTION_LIMIT = 6


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(args, full_last_pass):
    env = {k: v for k, v in os.environ.items() if k != "NGICP_FULL_LAST_PASS"}
    if full_last_pass:
        env["NGICP_FULL_LAST_PASS"] = "1"
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    res = subprocess.run([sys.executable, WORKER, *args], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert out["full_last_pass"] == ("1" if full_last_pass else "")
    return out["scenarios"]


@pytest.fixture(scope="module")
def runs(hip_lib):
    """(as built, NGICP_FULL_LAST_PASS=1): scenario name -> record"""
    return _worker(["main"], False), _worker(["main"], True)


@pytest.fixture(scope="module")
def sharded_runs(hip_lib):
    return _worker(["sharded", str(_free_port())], False), _worker(["sharded", str(_free_port())], True)


def _pair(runs, name, lm=True):
    """The scenario's two records, compared bit for bit; lm: the alignment made LM trials, so its last pass at least was K4-only."""
    d, f = runs[0][name], runs[1][name]
    print(f"{name}: passes {d['passes']}, search_passes {d['search_passes']} (switch: {f['search_passes']}), iterations {d['iters']}, converged {d['converged']}, "
          f"valid_fraction {d.get('valid_fraction')} / {f.get('valid_fraction')}, mean_candidates {d.get('mean_candidates')} / {f.get('mean_candidates')}")
    for key in BIT_EQUAL:
        if key in d:
            assert d[key] == f[key], f"{name}: {key} differs between the default and NGICP_FULL_LAST_PASS=1"
    assert f["search_passes"] == f["passes"], name
    if lm:
        assert d["passes"] == d["lm_trials"] + 1
        assert 0 < d["search_passes"] < d["passes"], name
    else:
        assert d["search_passes"] == d["passes"], name
    return d, f


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("limit", [1, 2, 5])
def test_iteration_limit(runs, shape, limit):
    """max_iterations 1, 2, 5 with eps 1e-12: every trial of the last outer iteration is case 2 of the rule."""
    d, _ = _pair(runs, f"{shape}/limit{limit}")
    assert d["iters"] == limit - 1 and not d["converged"]
    last = [r for r in d["trace_rows"] if r[0] == limit - 1]
    assert d["passes"] - d["search_passes"] == len(last)  # exactly the trials of the last outer iteration


@pytest.mark.parametrize("shape", SHAPES)
def test_convergence_by_epsilon(runs, shape):
    """DLO's eps 0.01, limit 32: the trial whose step meets the convergence test (case 1) ends the alignment."""
    d, _ = _pair(runs, f"{shape}/epsilon")
    assert d["converged"] and d["iters"] < 31
    assert d["search_passes"] == d["passes"] - 1


def test_rejected_trial_in_the_last_outer_iteration(runs, oracle_mod):
    """10k scan-to-scan from its usual guess, eps 1e-12, limit 6: the alignment reaches its noise floor in outer iteration 5, where
    the trials' gain ratios are rounding noise and most are rejected (the CPU oracle's trace, run on one thread when these inputs
    were fixed: ten rejected trials in iteration 5; checked again below).  After each rejected trial the alignment goes on,
    after a K4-only pass, from the same linearisation."""
    from _terminal_pass_worker import EPS12, shapes
    src, tgt, guess = shapes()["10k_10k"]
    o = oracle_mod.OracleGICP()
    o.setNumThreads(1)  # (one thread: its sums, and with them the noise-floor decisions, are the same in every run)
    o.setCorrespondenceRandomness(20)
    o.setMaxCorrespondenceDistance(1.0)
    o.setMaximumIterations(REJECTION_LIMIT)
    for name, v in EPS12.items():
        getattr(o, name)(v)
    o.setInputSource(src)
    o.setInputTarget(tgt)
    o.align(np.asarray(guess, np.float32))
    tr = o.lm_trace()
    last = tr[tr[:, 0] == REJECTION_LIMIT - 1]
    print(f"oracle: {len(last)} trials in outer iteration {REJECTION_LIMIT - 1}, {int((last[:, 7] == 0).sum())} rejected")
    assert (last[:-1, 7] == 0).any(), "the oracle's trace shows no rejection followed by another trial in the last outer iteration"
    d, _ = _pair(runs, "10k_10k/rejection")
    rows = [r for r in d["trace_rows"] if r[0] == REJECTION_LIMIT - 1]
    print(f"engine: {len(rows)} trials in outer iteration {REJECTION_LIMIT - 1}, {sum(1 for r in rows if r[2] == 0)} rejected")
    assert any(r[2] == 0 for r in rows[:-1]), "the engine's trace has no rejected trial followed by another in the last outer iteration"
    assert d["passes"] - d["search_passes"] == len(rows)  # every one of them was a K4-only pass


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lm_max", [1, 2])
def test_lm_max_iterations(runs, shape, lm_max):
    """lm_max_iterations 1 and 2 at the limit of the rejection test: the first (two) rejected trial(s) end the alignment with "lm not
    converged" (10k: in the last outer iteration, behind K4-only passes)."""
    d, _ = _pair(runs, f"{shape}/lm_max{lm_max}")
    assert all(r[1] < lm_max for r in d["trace_rows"])


@pytest.mark.parametrize("shape", SHAPES)
def test_gauss_newton(runs, shape):
    d, _ = _pair(runs, f"{shape}/gauss_newton", lm=False)
    assert d["lm_trials"] == 0 and d["passes"] >= 2


@pytest.mark.parametrize("shape", SHAPES)
def test_robust_kernel(runs, shape):
    _pair(runs, f"{shape}/huber")


@pytest.mark.parametrize("shape", SHAPES)
def test_after_swap(runs, shape):
    _pair(runs, f"{shape}/swapped")


def test_sharded_loop(sharded_runs):
    for name in ("10k_10k/sharded_epsilon", "10k_10k/sharded_limit2"):
        d, f = _pair(sharded_runs, name)
        assert d["equals_align"] and f["equals_align"] and d["passes"] == d["align_passes"]


def _solver_order(costs):
    """k_lm_solve's launch order of the groups with these costs (ngicp_solve.h build_launch_order): sixteen classes relative to the slowest
    group, heaviest class first, ascending group index inside a class; float32 arithmetic as on the device."""
    c = np.asarray(costs, np.int32)
    to_class = np.float32(16.0) / (np.float32(max(1, int(c.max()))) + np.float32(1.0))
    cls = 15 - np.minimum(15, (c.astype(np.float32) * to_class).astype(np.int32))
    return np.argsort(cls, kind="stable")


@pytest.mark.parametrize("shape", SHAPES)
def test_two_alignments_in_a_row(runs, shape):
    d1, f1 = _pair(runs, f"{shape}/first_of_two")
    _pair(runs, f"{shape}/second_of_two")
    sums = []
    for label, r in (("default", d1), ("NGICP_FULL_LAST_PASS=1", f1)):
        costs, order = np.array(r["costs"]), np.array(r["order"])
        print(f"{shape} {label}: {len(costs)} groups, cost sum {int(costs.sum())}, min {int(costs.min())}, max {int(costs.max())}")
        assert sorted(order.tolist()) == list(range(len(costs))), f"{label}: the launch order is no permutation of the groups"
        assert np.array_equal(order, _solver_order(costs)), f"{label}: the launch order is not the sort of the costs in the buffer"
        assert costs.min() > 0
        sums.append(float(costs.sum()))
    assert 0.5 < sums[0] / sums[1] < 2.0, f"cost sums {sums}: one mode's launch order was built from a pass that did not search"
    print(f"{shape}: staged_fraction of the first alignment {d1['staged_fraction']:.4f} / {f1['staged_fraction']:.4f}")
    assert (d1["staged_fraction"] >= 0.12) == (f1["staged_fraction"] >= 0.12)


@pytest.mark.parametrize("shape", SHAPES)
def test_statistics_of_a_two_pass_alignment(runs, shape):
    """max_iterations = 1: two passes, one of them K4-only - where dividing by `passes` would have halved the means."""
    d, f = _pair(runs, f"{shape}/limit1")
    assert d["passes"] == 2 and d["search_passes"] == 1
    for r in (d, f):
        assert 0.5 < r["valid_fraction"] <= 1.0 and r["mean_candidates"] > 0
