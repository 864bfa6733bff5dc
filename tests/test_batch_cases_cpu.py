"""The yardstick of the batched-alignment tests, on the CPU oracle alone: the guess set of tests/_batch_cases.py really does spread
its lanes over very different iteration counts, so a batch cannot pass test_gpu_batch.py on lanes that all happen to stop together;
and "lowest fitness" really does pick a correctly aligned lane (the recipe of INTEGRATION.md, "More than one candidate pose")."""
import numpy as np
import pytest

import _batch_cases as bc


@pytest.fixture(scope="module")
def runs(oracle_mod):
    w = bc.workload()
    G = bc.guesses(w)
    out = {}
    for max_iter in (32, 8):
        o = oracle_mod.OracleGICP()
        o.setNumThreads(16)
        bc.configure(o, max_iter)
        o.setInputSource(w.source)
        o.setInputTarget(w.target)
        res = []
        for g in G:
            o.align(g)
            res.append((o.final_transformation.copy(), bool(o.converged), int(o.nr_iterations)))
        out[max_iter] = res
    return w, G, out


def test_guess_set_shape(runs):
    _, G, _ = runs
    assert G.shape == (12, 4, 4) and G.dtype == np.float32


def test_iteration_counts_are_spread(runs):
    _, _, out = runs
    its = [r[2] for r in out[32]]
    print("oracle iterations at max_iter = 32:", its, "converged:", [r[1] for r in out[32]])
    assert len(set(its)) >= 5
    assert 0 in its
    assert max(its) >= 20


def test_short_budget_cuts_some_lanes_off(runs):
    _, _, out = runs
    conv = [r[1] for r in out[8]]
    print("oracle at max_iter = 8: iterations", [r[2] for r in out[8]], "converged", conv)
    assert conv.count(False) >= 2
    assert conv.count(True) >= 6


@pytest.mark.parametrize("max_range", [None, 1.0])
def test_lowest_fitness_is_a_correct_lane(runs, oracle_mod, max_range):
    w, _, out = runs
    scores = [bc.oracle_fitness(oracle_mod, w, r[0], max_range) for r in out[32]]
    print("oracle fitness, max_range =", max_range, ":", ["%.4g" % s for s in scores])
    assert int(np.argmin(scores)) in bc.GOOD_LANES
    assert max(scores[g] for g in bc.GOOD_LANES) < min(s for g, s in enumerate(scores) if g not in bc.GOOD_LANES)
